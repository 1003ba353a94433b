"""Every launch site that reads the non-temporal knob has tests that run both of its arms.

A launch site that reads g_tune.nontemporal ships two instantiations of its kernels (NT and
cached) per vector-path shape.  TABLE names, for every source file under csrc/ with such a
site, the test functions that run it with the knob at 0 and at 1.  A new file that reads the
knob fails this test until someone names the tests that run both of its arms; a renamed or
removed test fails it too.  No GPU is used: the sources and the test modules are only read.
"""
import ast
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vsiquantization_amd", "csrc")
TESTS = os.path.join(ROOT, "tests")

D, X, PAR = "test_gpu_dispatch", "test_gpu_dispatch_ext", "test_gpu_parity"
BOTH = "both"   # one test function that crosses the knob itself (parametrised or looped over 1 and 0)

# file -> {knob value or BOTH: [(test module, test function), ...]}
TABLE = {
    "k_fq.cuh": {BOTH: [(D, "test_fq_fwd_and_ste_bwd")],
                 0: [(X, "test_half_forward_every_input_value_cached_arm"), (X, "test_half_edges_cached_arm")]},
    "k_ste.cuh": {BOTH: [(D, "test_fq_fwd_and_ste_bwd")],
                  0: [(X, "test_half_ste_backward_cached_arm"), (X, "test_half_edges_cached_arm")]},
    "k_lsq.cuh": {BOTH: [(D, "test_lsq_bwd")],
                  0: [(X, "test_half_lsq_backward_cached_arm"), (X, "test_half_edges_cached_arm")]},
    "k_lsq.hip": {BOTH: [(D, "test_pc_lsq_bwd_rows_in_registers"), (D, "test_pc_lsq_bwd_channel_columns")]},
    "k_pc.hip": {BOTH: [(PAR, "test_nontemporal_off_equals_default"), (X, "test_pc_fixed_fake_quant")]},
    "k_act.hip": {BOTH: [(D, "test_act_fwd_bwd")]},
    "k_observe.hip": {BOTH: [(D, "test_observe_parts"), (D, "test_observe_parts_out")]},
    "k_observe_fq.hip": {BOTH: [(D, "test_observe_fq")]},
    # K2 and the two second passes take the NT arm only from 256 MB with the knob on
    "k_observe_k2.cuh": {1: [(D, "test_observe_nontemporal")],
                         0: [(D, "test_observe"), (PAR, "test_nontemporal_off_equals_default")]},
    "k_observe_mse.hip": {1: [(X, "test_mse_observer_nt_arm_equals_host"),
                              (X, "test_mse_observer_nt_arm_all_candidates")],
                          0: [(X, "test_mse_observer_cached_arm_at_the_full_grid")]},
    "k_observe_hist.hip": {1: [(X, "test_percentile_observer_nt_arm_equals_host"),
                               (X, "test_percentile_observer_nt_arm_other_bin_counts")],
                           0: [(X, "test_percentile_observer_cached_arm_at_the_full_grid")]},
    "k_pc_mse.hip": {BOTH: [(X, "test_pc_mse_observer")]},
    "k_pack.hip": {BOTH: [(X, "test_pack_unpack")]},
    "k_adaround.hip": {BOTH: [(X, "test_adaround_vector_shapes")], 0: [(X, "test_adaround_cached_arm")]},
    "k_multi.hip": {1: [("test_gpu_multi", "test_multi_equals_per_tensor")], 0: [(X, "test_lsq_multi_cached_arm")]},
}

# a read of the knob: the name not followed by an assignment (k_lib.hip's setter writes it)
READ = re.compile(r"g_tune\.nontemporal\b(?!\s*=[^=])")


def _readers():
    out = set()
    for name in sorted(os.listdir(CSRC)):
        with open(os.path.join(CSRC, name)) as f:
            if READ.search(f.read()):
                out.add(name)
    return out


def _functions(module):
    """(names of the module's top-level functions, its text), from the file (no import)."""
    path = os.path.join(TESTS, module + ".py")
    text = open(path).read()
    return {n.name for n in ast.parse(text, path).body if isinstance(n, ast.FunctionDef)}, text


def test_the_pattern_tells_reads_from_writes():
    assert READ.search("const bool nt = g_tune.nontemporal != 0;")
    assert READ.search("launch(act, vec, g_tune.nontemporal != 0, c);")
    assert READ.search("if (g_tune.nontemporal == 0) return;")
    assert not READ.search("case VSIQ_TUNE_NONTEMPORAL: g_tune.nontemporal = value; return 0;")
    assert "k_lib.hip" not in _readers() and len(_readers()) >= 15


def test_every_launch_site_that_reads_the_knob_is_listed():
    readers = _readers()
    assert readers == set(TABLE), {"not listed": sorted(readers - set(TABLE)), "stale": sorted(set(TABLE) - readers)}


def test_both_arms_of_every_listed_file_have_tests_that_exist():
    for name, arms in TABLE.items():
        assert arms and set(arms) <= {0, 1, BOTH}, name
        assert BOTH in arms or {0, 1} <= set(arms), (name, "one arm has no test")
        for arm, tests in arms.items():
            assert tests, (name, arm)
            for module, fn in tests:
                fns, text = _functions(module)
                assert fn in fns and fn.startswith("test_"), (name, module, fn)
                if arm in (0, BOTH):   # the knob leaves its default only where a test says so
                    assert "NONTEMPORAL" in text, (name, module)
