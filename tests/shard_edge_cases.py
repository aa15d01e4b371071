"""The shapes of tests/test_gpu_shard_edges.py (row-strip shards on thin strips and under every level schedule), and
what each one is there for.  tests/test_shard_edges_cpu.py asserts with the host-only planners that the shapes reach
it; nothing here touches a device."""
from collections import namedtuple

# reaches: what the JumpFlood exchange plan of the shape must show (test_shard_edges_cpu.py)
#   "all_block"      every step 1 .. S-1 is a block step, the last included.  Only one-row strips can: the last
#                    step shifts by one row, and a strip of two rows or more takes that (plus the rounding margin
#                    of a non-power-of-two screen, on strips of three rows or more) as a halo of its window
#   "same_block"     a step whose two shifted taps read one block buffer (both shifts round to the same row)
#   "three_sources"  a block request served by three or more owners (the `while (done < nd.n)` loop of
#                    plan_jfa_exchange): a strip plus its rounding margin spans three strips
# Every thin shape has a block step, and a rank that awaits four or more peers before some step.
Thin = namedtuple("Thin", "W H N rr rs blur world linux_merge heights reaches what")

THIN = [
    Thin(64, 40, 3, 2.0, 1.0, 1.5, 40, False, {1}, {"all_block", "three_sources"},
         "one-row strips, float taps with rounding margin 1, separate blur passes"),
    Thin(128, 64, 4, 2.0, 1.0, 1.5, 64, False, {1}, {"all_block"},
         "one-row strips on the fused blur + merge: strip-sized textures of one row"),
    Thin(128, 64, 4, 2.0, 1.0, 1.5, 32, False, {2}, set(), "two-row strips on the fused blur + merge"),
    Thin(128, 64, 4, 2.0, 1.0, 1.37, 32, False, {2}, set(), "LDS-tiled blur"),
    Thin(128, 64, 4, 2.0, 1.0, 0.0, 32, False, {2}, set(), "blur off"),
    Thin(96, 50, 3, 2.0, 1.0, 2.5, 16, False, {3, 4}, {"three_sources"}, "strips of 3 and 4 rows, CH = 56 != H"),
    Thin(128, 64, 3, 2.0, 0.5, 1.5, 16, False, {4}, set(), "cascade coarser than the screen"),
    Thin(96, 50, 3, 2.0, 1.7, 1.5, 16, False, {3, 4}, {"three_sources"}, "cascade finer than the screen"),
    Thin(64, 64, 1, 2.0, 1.0, 1.5, 64, False, {1}, {"all_block"}, "a screen larger than 3 x 2 with N = 1"),
    Thin(128, 64, 4, 2.0, 1.0, 1.5, 32, True, {2}, set(), "raylib's merge shader missing: no strip-sized textures"),
    # taller than wide and not a power of two: the last step's offset is below half a row, its three taps read the
    # same rows and share one block buffer (no shape with W >= H has such a step)
    Thin(24, 64, 2, 2.0, 1.0, 1.5, 64, False, {1}, {"all_block", "same_block", "three_sources"},
         "one-row strips whose last step reads one block for both shifted taps"),
]
STORAGES = ("f32", "f16", "rgba8")


def thin_id(t):
    return (f"{t.W}x{t.H}-N{t.N}-rs{t.rs:g}-blur{t.blur:g}-w{t.world}" + ("-linuxmerge" if t.linux_merge else ""))


# W, H, N, rayRange, blur, world: every tile variant, proof, order and blur path under a row window
Sweep = namedtuple("Sweep", "W H N rr blur world")
SWEEPS = [Sweep(256, 256, 5, 2.0, 1.5, 3),   # strips of 85 / 85 / 86 rows
          Sweep(333, 200, 4, 2.0, 1.5, 3)]   # a cascade that is no power of two (336 x 208)
# the top levels start off screen: launch_rc_fill on the rows of an unbanded shard
FILL = Sweep(512, 512, 8, 64.0, 1.5, 3)

# rc_order_L<n> codes: tile-major; patches; one-tile patches of 16 groups; oriented; bands; the patch code with the
# XCD interleave lc = 2 and lc = 16 in bits 26-30; a patch that tiles nothing
ORDER_CODES = [0, 2 | 2 << 8 | 8 << 16, 1 | 16 << 8 | 16 << 16, 2 | 2 << 8 | 4 << 16 | 1 << 24,
               2 | 2 << 8 | 4 << 16 | 2 << 24, 2 | 2 << 8 | 8 << 16 | 2 << 26, 2 | 2 << 8 | 8 << 16 | 16 << 26,
               2 | 3 << 8 | 5 << 16]


def strip(H, rank, world):
    return rank * H // world, (rank + 1) * H // world

