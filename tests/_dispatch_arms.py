"""The census of the dispatchers in zinc_amd/csrc/zip_hip.hip: per dispatcher, every arm and the test that runs it.

Data only.  tests/test_dispatch_census.py holds it to the source: the `case` / `default` labels of every function in
SWITCHES must be exactly the keys listed here, and every test named must exist.  An arm added to a switch without an
entry here fails that test; so does an entry whose test was renamed away.

An entry is (node, selects) or (node, selects, note):
    node     "tests/<file>.py::<test function>", or None for an arm that no caller can reach (the note says why)
    selects  the parameter value or knob of that test which picks the arm
A switch label is the text between `case` and `:`; the `default:` arm is keyed "default" and its note says which value
it stands for.
"""

_ARMS = "tests/test_gpu_dispatch_arms.py::"
_WALK = "tests/test_gpu_gather_walk.py::test_scalar_gather_writes_the_oracles_openings"
_VARIANTS = "tests/test_gpu_gather_variants.py::test_gather_variant_writes_the_oracles_proof"
_LARGE_GATHER = "tests/test_gpu_gather_variants.py::test_large_codeword_gather_variants"
_COMMIT = "tests/test_gpu_parity.py::test_commit_bit_exact"
_CODES = "tests/test_gpu_batch_codes.py::test_commit_codes_equals_oracle_per_member"
_SHARD_ROWS = "tests/test_gpu_large_codewords.py::test_commit_row_shard_matches_oracle"
_T_OPEN = "tests/test_gpu_proximity_open.py::test_open_on_a_plain_handle"
_T_NEW = _ARMS + "test_open_with_four_to_seven_proximity_tests"
_ONE = _ARMS + "test_sumcheck_one_thread_arms"
_QUAD = _ARMS + "test_sumcheck_quad_arms"
_WIDE = "tests/test_gpu_sumcheck_wide.py::test_rounds_equal_the_oracle"
_MERKLE = _ARMS + "test_merkle_trees_every_leaf_width_and_split"
_SUM_F = _ARMS + "test_sum_partials_field_halves"

# ---- the `switch` dispatchers, by the name of the enclosing function ----------------------------------------------------
SWITCHES = {
    # switch (g.e): entries per thread of the commit kernel, from commit_geom(cw, row_len)
    "dispatch_commit": {
        "64": (_SHARD_ROWS, "nv=29: cw 65536 (shares the slab kernel's arm with 32)"),
        "32": (_SHARD_ROWS, "nv=27: cw 32768"),
        "16": ("tests/test_gpu_parity.py::test_commit_extreme_witnesses", "geometry (17, (8192, 16, 16384)): cw 16384"),
        "8": (_COMMIT, "num_vars=16: cw 512"),
        "4": (_COMMIT, "num_vars=13: cw 256"),
        "2": (_COMMIT, "num_vars=12: cw 128"),
        "default": (_COMMIT, "num_vars=10: cw 64", "g.e == 1, every cw <= 64"),
    },
    # switch (g.e) of zip_batch_commit_codes: a code per member
    "dispatch_commit_codes": {
        "8": (_CODES, "num_vars=15: cw 512"),
        "4": (_CODES, "num_vars=13: cw 256"),
        "2": (_CODES, "num_vars=12: cw 128"),
        "1": (_CODES, "num_vars=8: cw 32"),
        "default": (None, "cw > 8192",
                    "unreachable: the batch commit refuses `codes && cw > kMaxCodesCodeword` before it dispatches "
                    "(tests/test_gpu_batch_codes.py::test_usage_errors_reach_no_device sees that refusal)"),
    },
    # switch (nt): proximity tests beside the first, combine_rows_extra_kernel<nt>; nt = T - 1
    "run_combine_extra": {
        "1": (_T_OPEN, "T=2"),
        "2": (_T_OPEN, "T=3"),
        "3": (_T_NEW, "T=4"),
        "4": (_T_NEW, "T=5"),
        "5": (_T_NEW, "T=6"),
        "6": (_T_NEW, "T=7"),
        "default": (_T_OPEN, "T=8", "nt == 7; more is refused above the switch"),
    },
    # switch (ctx->depth): open_columns_ilv_scalar_kernel<P, depth>, P = 2 when a block has 64 rows
    "run_open_columns": {
        "12": (_WALK, "geometry B; knob none: <1, 12>, rpb64: <2, 12>"),
        "13": (_WALK, "geometry C; knob none: <1, 13>, rpb64: <2, 13>"),
        "default": (_WALK, "geometry D; knob image32: <1, 14>, image64: <2, 14>",
                    "depth 14: the `if` above the switch admits 12 .. 14 only.  image64 (STREAM=0 RPB=64) does select "
                    "two == true: rpb = 64, the commit of D is one chunk of 64 rows (one workgroup of the 16-entry "
                    "kernel per CU, so no priority classes), and 64 * pk_stride <= 64 * 112 KiB for 1000 openings"),
    },
    # switch (s->degree)
    "sumcheck_round_k": {
        "1": (_ONE, "degree=1"),
        "2": (_ONE, "degree=2"),
        "3": (_ONE, "degree=3"),
        "default": (_ONE, "degree=4", "zip_sumcheck_init admits 1 .. 4"),
    },
    # switch (s->n_mles)
    "sumcheck_round_fl": {
        "1": (_ONE, "K=1"),
        "2": (_ONE, "K=2"),
        "3": (_ONE, "K=3"),
        "4": (_ONE, "K=4"),
        "5": (_WIDE, "K=5"),
        "6": (_WIDE, "K=6"),
        "7": (_WIDE, "K=7"),
        "default": (_WIDE, "K=8", "zip_sumcheck_init admits 1 .. 8"),
    },
    # switch (leaf_limbs): merkle_leaves_kernel<limbs>
    "zip_merkle_trees": {
        "1": (_MERKLE, "limbs=1"),
        "2": (_MERKLE, "limbs=2"),
        "3": (_MERKLE, "limbs=3"),
        "4": (_MERKLE, "limbs=4"),
        "5": (_MERKLE, "limbs=5"),
        "6": (_MERKLE, "limbs=6"),
        "7": (_MERKLE, "limbs=7"),
        "default": (_MERKLE, "limbs=8", "the entry point refuses limbs > 8"),
    },
    # switch (fl): here for sum_partials_kernel<FL>, the kernel this census adds limb counts for (WITH_FL below has the
    # other kernels; kernel x FL is not enumerated)
    "with_fl": {
        "2": (_SUM_F, "modulus 2^128 - 159"),
        "3": (_SUM_F, "MOD_3LIMB"),
        "default": (_SUM_F, "MOD_NO_SPARE", "fl == 4: make_field admits 2, 3, 4"),
    },
}

# sumcheck_round_k x sumcheck_round_fl: the (K, degree) instances of sumcheck_round_kernel and of
# sumcheck_round_quad_kernel per limb count.  Every pair of 1..4 x 1..4 runs in _ONE under ZIP_HIP_SUMCHECK_QUAD=0 and every
# pair with degree 2 or 3 in _QUAD under =2, for FL = 2, 3, 4; zip_sumcheck_init refuses no pair of that range.
SUMCHECK_PAIRS = {
    "sumcheck_round_kernel": (_ONE, "K in 1..4, degree in 1..4"),
    "sumcheck_round_quad_kernel": (_QUAD, "K in 1..4, degree in {2, 3}"),
}

# kernels reached through with_fl for which this census pins a limb count or a quirk modulus (2^(64 FL) - q < 2^64)
WITH_FL = {
    "sum_partials_kernel": {
        "2": (_SUM_F, "modulus 2^128 - 159 (no spare bit: the carry branch)"),
        "3": (_SUM_F, "MOD_3LIMB"),
        "4": (_SUM_F, "MOD_NO_SPARE (the carry branch)"),
        "through zip_mctx": (_ARMS + "test_three_shards_on_one_device", "(MOD_3LIMB, 3), (MOD_NO_SPARE, 4)"),
    },
    "field_map_i64_kernel with quirk_mod": {
        "2": (_ARMS + "test_quirk_ccs_tables_equal_the_oracle", "modulus 2^128 - 159"),
        "3": (_ARMS + "test_quirk_ccs_tables_equal_the_oracle", "modulus 2^192 - 237"),
        "4": ("tests/test_gpu_spartan.py::test_ccs_tables_equal_the_oracle", "Q256"),
    },
}

# ---- the if / else dispatchers, by hand ---------------------------------------------------------------------------------
IF_ELSE = {
    # run_combine_fl, per FL:
    #   if (a.quirk_mod && do_field) { if (do_int) <FL, true, true, true> else <FL, false, true, true> }
    #   else if (do_int && do_field) <FL, true, true, false>
    #   else if (do_int)             <FL, true, false, false>
    #   else                         <FL, false, true, false>
    "run_combine_fl: combine_rows_kernel": {
        "<FL, true, true, true>": (_ARMS + "test_quirk_open_runs_both_row_combinations", "FL 2, 3 (zip_open)",
                                   "FL 4: tests/test_gpu_parity.py::test_full_open_proof_equals_oracle_and_verifies"),
        "<FL, false, true, true>": (_ARMS + "test_quirk_open_eval_alone", "FL 2, 3 (zip_open_eval)",
                                    "FL 4: tests/test_gpu_parity.py::test_open_eval_bit_exact with MOD_NO_SPARE"),
        "<FL, true, true, true> on a row shard": (_ARMS + "test_three_shards_on_one_device", "(MOD_NO_SPARE, 4)"),
        "<FL, true, true, false>": ("tests/test_gpu_parity.py::test_full_open_proof_equals_oracle_and_verifies", "every modulus but MOD_NO_SPARE"),
        "<FL, true, false, false>": ("tests/test_gpu_parity.py::test_open_testing_bit_exact", "any (no field: FL is 4)"),
        "<FL, false, true, false>": ("tests/test_gpu_parity.py::test_open_eval_bit_exact", "every modulus but MOD_NO_SPARE"),
    },
    # run_combine_fl:
    #   if (do_int && do_field) <FL, true, true> else if (do_int) <FL, true, false> else <FL, false, true>
    "run_combine_fl: combine_finalize_kernel": {
        "<FL, true, true>": ("tests/test_gpu_parity.py::test_full_open_proof_equals_oracle_and_verifies", "any"),
        "<FL, true, false>": ("tests/test_gpu_parity.py::test_open_testing_bit_exact", "any"),
        "<FL, false, true>": ("tests/test_gpu_parity.py::test_open_eval_bit_exact", "any"),
    },
    # merkle_upper_levels, from level 0 of zip_merkle_trees (rem = depth - level):
    #   if (rem >= 4) launch_upper<4> else if (rem == 3) <3> else if (rem == 2) <2> else <1>;  depth == 0: copy_roots_depth0_kernel
    "merkle_upper_levels": {
        "launch_upper<4>": (_MERKLE, "depth 5, 7, 9 (first pass)"),
        "launch_upper<3>": (_MERKLE, "depth 3 from level 0; depth 7 after one pass of 4"),
        "launch_upper<2>": (_MERKLE, "depth 2 from level 0"),
        "launch_upper<1>": (_MERKLE, "depth 1 from level 0; depths 5 and 9 after passes of 4"),
        "copy_roots_depth0_kernel": (_MERKLE, "depth 0"),
    },
    # run_open_columns, natural layout:
    #   if (stream && ctx->depth >= 1 && 2 * ctx->depth + 3 <= 64) { if (2 * ctx->depth + 3 <= 32) stream<32> else stream<64> }
    #   else if (2 * ctx->depth + 1 <= 32) open_columns_kernel<32> else open_columns_kernel<64>
    "run_open_columns: natural layout": {
        "open_columns_kernel<32>": (_VARIANTS, "path plain, knob none, geometries A, B, C"),
        "open_columns_kernel<64>": (_LARGE_GATHER, "key cw65536 (depth 16), knob none"),
        "open_columns_stream_kernel<32>": (_VARIANTS, "path plain, knob stream"),
        "open_columns_stream_kernel<64>": (_LARGE_GATHER, "knob stream (depth 15 and 16)"),
    },
    # launch_sumcheck_round, DEG 2 or 3:
    #   pays = a.fold && (DEG == 3 || a.half <= 65536u);  if (mode == 2 || (mode == 1 && pays)) quad kernel, else one thread per point
    "launch_sumcheck_round": {
        "sumcheck_round_quad_kernel": (_QUAD, "ZIP_HIP_SUMCHECK_QUAD=2: every round"),
        "sumcheck_round_kernel": (_ONE, "ZIP_HIP_SUMCHECK_QUAD=0: every round"),
        "the default choice (mode 1)": ("tests/test_gpu_sumcheck.py::test_degree_3_rounds_on_both_kernels", "quad=1"),
    },
}

# ---- arms that were reachable but run by no test before this census, and what runs them now ---------------------------
CLOSED = {
    "combine_rows_extra_kernel<3..6>": (_T_NEW, "T in 4..7, num_vars 13 and 16"),
    "combine_rows_extra_kernel<3..6> at the accumulator bound": (_ARMS + "test_open_testing_at_the_accumulator_bound", "T in 4..7"),
    "verify_extra_tests_kernel with 3..6 tests": (_ARMS + "test_verify_with_four_to_seven_proximity_tests", "T in 4..7"),
    "field_from_int256 with a 2- / 3-limb quirk modulus on zip_verify": (_ARMS + "test_quirk_proof_mle_eval_and_verdict", "both moduli"),
    "field_from_i64 with quirk_mod inside a single zip_ccs": (_ARMS + "test_quirk_ccs_tables_equal_the_oracle", "both moduli"),
    "open_columns_ilv_scalar_kernel<2, 14>": (_WALK, "D-image64-13, D-image64-1000"),
    "sum_partials_kernel: 512-bit carries": (_ARMS + "test_sum_partials_integer_halves", "G in {1, 3, 4}"),
}
