"""CPU: RC2DGI_RCCL_LIB names the transport library rc2dgi_group.cpp opens in place of librccl.so.1.  The variable is
read once per process, at the first use of the transport, so every check runs in a child process of its own; the
child loads librc2dgi.so alone (no torch, which would bring the real RCCL with it) and touches no device."""
import os
import shutil
import subprocess
import sys

import pytest

from rccl_ranks_worker import standin_library

E_UNSUPPORTED = -5
CHILD = """
import ctypes, sys
L = ctypes.CDLL(sys.argv[1])
buf = ctypes.create_string_buffer(128)
print(L.rc2dgi_shard_unique_id(buf, 128), buf.raw[:8].decode("latin-1"))
"""


@pytest.fixture(scope="module")
def lib():
    from radiancecascade2dglobalillumination_amd import _build

    return _build.build()


@pytest.fixture(scope="module")
def standin(tmp_path_factory):
    return standin_library(tmp_path_factory.mktemp("fake_rccl"))


def unique_id_in_child(lib, **env):
    e = {k: v for k, v in os.environ.items() if k != "RC2DGI_RCCL_LIB"}
    e.update({k: v for k, v in env.items() if v is not None})
    p = subprocess.run([sys.executable, "-c", CHILD, lib], env=e, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    rc, _, magic = p.stdout.strip().partition(" ")
    return int(rc), magic


def test_named_standin_makes_the_unique_id(lib, standin):
    assert unique_id_in_child(lib, RC2DGI_RCCL_LIB=standin) == (0, "FAKERCCL")


@pytest.mark.parametrize("named", ["/nonexistent/librccl_named.so", "libm.so.6"], ids=["missing", "lacks-symbols"])
def test_named_library_that_cannot_serve_is_unsupported(lib, standin, tmp_path, named):
    """No fallback to the library's default name: a librccl.so.1 that would serve is first on the loader's path."""
    shutil.copy(standin, tmp_path / "librccl.so.1")
    path = os.pathsep.join(filter(None, [str(tmp_path), os.environ.get("LD_LIBRARY_PATH")]))
    assert unique_id_in_child(lib, RC2DGI_RCCL_LIB=named, LD_LIBRARY_PATH=path)[0] == E_UNSUPPORTED


@pytest.mark.parametrize("value", [None, ""], ids=["unset", "empty"])
def test_unset_opens_librccl_by_name_as_before(lib, standin, tmp_path, value):
    """Unset (or empty, as RC2DGI_LIB): dlopen("librccl.so.1") by name, through the loader's search path -- shown by
    putting a copy of the stand-in under that name first on the path; its ids carry its mark."""
    shutil.copy(standin, tmp_path / "librccl.so.1")
    path = os.pathsep.join(filter(None, [str(tmp_path), os.environ.get("LD_LIBRARY_PATH")]))
    assert unique_id_in_child(lib, RC2DGI_RCCL_LIB=value, LD_LIBRARY_PATH=path) == (0, "FAKERCCL")
