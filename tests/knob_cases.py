"""Every settable tuning key (include/rc2dgi.h) with one valid value that is not its default at any level, for the
round-trip tests of tests/test_gpu_parity.py.  "<n>" stands for a level.  tests/test_tuning_files_cpu.py asserts that
the keys are exactly the library's table (tests/sanitize/tuning_check --list)."""

KNOB_CASES = [
    ("strip_tables", 0),
    ("rc_variant", 17),
    ("rc_variant_L<n>", 5),
    ("blur_path", 2),
    ("poison", 1),
    ("rc_skip", 3),
    ("rc_wgproof", 0),
    ("cascade_band", 0),
    ("rc_fill", 0),
    ("rc_rdiv", 0),
    ("jfa_tab", 0),
    ("jfa_tail", 2),
    ("jfa_coset", 0),
    ("shade_fused", 0),
    ("shade_split", 0),
    ("side_overlap", 1),
    ("jfa_lds", 1),
    ("jfa_rows", 4),
    ("jfa_rt", 2),
    ("rc_mp", 0),
    ("rc_mp_L<n>", 0),
    ("rc_tail", 3),
    ("rc_tail_L<n>", 0),
    ("rc_pal", 0),
    ("rc_chain", 1),
    ("rc_chain_spin", 1000),  # (a positive poll count only: -1 makes every chained wait time out)
    ("paint_plan", 3 | 1 << 8),  # (tiles of 8 rows, batches of 2048: within 40 MiB of masks on every screen of the tests)
    ("rc_noproof_L<n>", 1),
    ("rc_order_L<n>", 2 | 4 << 8 | 4 << 16),
]
