"""Every instantiation of the group-wise kernels (csrc/k_pg.hip, csrc/k_pg_mse.hip) has a test
that runs it.

The launchers of these files pick a kernel instantiation from which outputs are asked for (or,
for the learnable backward, whether the zero point is learned), and the entry points pick a launch
form: the per-element (scalar) path, the vector path with one task per wave, the vector path with
kPgU tasks per wave (k_pg_mse: scalar / vector only).  This test reads the
``hipLaunchKernelGGL((k_pg_...<...>)`` sites, the forms ``with_pg_form`` lists (csrc/k_pg_wave.cuh)
and which launcher or kernel each ``with_pg_form(vec, `` / ``with_bool(vec, `` call reaches, crosses
them, and requires TABLE to name, for every instantiation, test functions that run it.  A new arm
or launch form fails it until someone names its tests; a removed arm, or a renamed or removed
test, fails it too.  No GPU is used and no test module is imported: the sources are read as text
(template arguments only, never compiled code) and the test modules parsed with ``ast``.
"""
import ast
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vsiquantization_amd", "csrc")
TESTS = os.path.join(ROOT, "tests")
FILES = ("k_pg_wave.cuh", "k_pg.hip", "k_pg_mse.hip")

SITE = re.compile(r"hipLaunchKernelGGL\(\((k_pg_\w+)<([^<>]*)>\)")     # a launch: kernel, template arguments
VIA = re.compile(r"\b(with_pg_form|with_bool)\(vec,[^;]*?\b((?:launch|k)_pg_\w+)<")   # a dispatcher, what it reaches
FORM = re.compile(r"\bf\(BoolC<(\w+)>\{\}, IntC<(\w+)>\{\}\)")             # a form with_pg_form lists
LAUNCHER = re.compile(r"^static void (launch_pg_\w+)\(", re.M)         # a launcher's definition
INSTANCE = re.compile(r"\bk_pg_\w+<")                                  # any instantiation at all
CALL = re.compile(r"\blaunch_pg_\w+<")                                 # any call of a launcher at all

SCALAR, VEC1, VECU, VECTOR = "scalar", "vector, 1 task per wave", "vector, kPgU tasks per wave", "vector"
FORMS = {("false", "1"): SCALAR, ("true", "1"): VEC1, ("true", "kPgU"): VECU}

# the arms by the template arguments behind VEC (and U): <QUANT, CODES, MASK>, <CODES, MASK>, <ZPL>
OBSERVE = {"false, false, false": "observe only", "true, false, false": "plain", "true, true, false": "codes only",
           "true, false, true": "mask only", "true, true, true": "codes + mask"}
FIXED = {"false, false": "plain", "true, false": "codes only", "false, true": "mask only", "true, true": "codes + mask"}
ZPL = {"false": "zero point as given", "true": "learned zero point"}
ARMS = {"k_pg_observe_fq": OBSERVE, "k_pg_fq_fwd": FIXED, "k_pg_ste_bwd": {"": "-"}, "k_pg_lsq_bwd": ZPL,
        "k_pg_mse": OBSERVE}

A, PG, LEARN, MSE = "test_gpu_pg_arms", "test_gpu_pg", "test_gpu_pg_learn", "test_gpu_pg_mse"
FORMS_OF = (A, "test_every_output_form_of_both_forward_kernels")     # scalar, offset view, 5 x 296 and the wide tensor
WIDTHS = (A, "test_four_tasks_per_wave_at_every_group_width")        # the wide tensor and the one just under it
CROSS = (A, "test_dense_small_cross")                                # vector and scalar row lengths, 1 task per wave
STE_EDGES = (A, "test_ste_backward_at_gradient_and_scale_edges")
K3_ROUTE = (PG, "test_kernels_equal_the_reshaped_k3_route_and_the_host_loops")
K3_FOUR = (PG, "test_four_tasks_per_wave_from_the_grid_size_threshold_on")
LSQ_ROUTE = (LEARN, "test_kernel_equals_the_oracle_the_host_loops_and_the_parent_route")
LSQ_FOUR = (LEARN, "test_four_tasks_per_wave_from_the_grid_size_threshold_on")
MSE_ARMS = (MSE, "test_every_output_arm")                             # rowlen 256 and 258

# (kernel, arm, launch form) -> [(test module, test function), ...]
TABLE = {}
for arm in OBSERVE.values():
    for form in (SCALAR, VEC1, VECU):
        TABLE[("k_pg_observe_fq", arm, form)] = [FORMS_OF]
    for form in (SCALAR, VECTOR):
        TABLE[("k_pg_mse", arm, form)] = [MSE_ARMS]
for arm in FIXED.values():
    for form in (SCALAR, VEC1, VECU):
        TABLE[("k_pg_fq_fwd", arm, form)] = [FORMS_OF]
for arm in ZPL.values():
    TABLE[("k_pg_lsq_bwd", arm, SCALAR)] = [CROSS, LSQ_ROUTE]
    TABLE[("k_pg_lsq_bwd", arm, VEC1)] = [CROSS, WIDTHS, LSQ_ROUTE]
    TABLE[("k_pg_lsq_bwd", arm, VECU)] = [WIDTHS, LSQ_FOUR]
TABLE[("k_pg_ste_bwd", "-", SCALAR)] = [STE_EDGES, CROSS, K3_ROUTE]
TABLE[("k_pg_ste_bwd", "-", VEC1)] = [STE_EDGES, CROSS, K3_ROUTE]
TABLE[("k_pg_ste_bwd", "-", VECU)] = [STE_EDGES, WIDTHS, K3_FOUR]
# the arms test_gpu_pg.py's _check_all already ran before test_gpu_pg_arms.py
for arm in ("observe only", "plain", "codes + mask"):
    for form, test in ((SCALAR, K3_ROUTE), (VEC1, K3_ROUTE), (VECU, K3_FOUR)):
        TABLE[("k_pg_observe_fq", arm, form)].append(test)
for form, test in ((SCALAR, K3_ROUTE), (VEC1, K3_ROUTE), (VECU, K3_FOUR)):
    TABLE[("k_pg_fq_fwd", "codes + mask", form)].append(test)
    TABLE[("k_pg_fq_fwd", "codes + mask", form)].append(CROSS if form != VECU else WIDTHS)


def _args(text):
    return tuple(a.strip() for a in text.split(","))


def instantiations(text):
    """{(kernel, arm, launch form)} of the source text.  A site inside a launcher (template
    arguments VEC, [U,] arm...) ships its arm in every form of the dispatcher whose lambda calls
    the launcher; a site inside such a lambda (decltype(V)::value, ...) in every form of that one."""
    launchers = [(m.start(), m.group(1)) for m in LAUNCHER.finditer(text)]
    listed = {"with_pg_form": {FORMS[m.groups()] for m in FORM.finditer(text)}, "with_bool": {SCALAR, VECTOR}}
    forms, calls = {}, 0
    for m in VIA.finditer(text):
        forms.setdefault(m.group(2), set()).update(listed[m.group(1)])
        calls += m.group(2).startswith("launch_pg_")
    assert calls == len(CALL.findall(text)), "a launcher called outside with_pg_form(vec, / with_bool(vec,"
    out, sites = set(), 0
    for m in SITE.finditer(text):
        sites += 1
        kernel, args = m.group(1), _args(m.group(2))
        owner = kernel if args[0] != "VEC" else [name for pos, name in launchers if pos < m.start()][-1]
        arm = ", ".join(a for a in args if a not in ("VEC", "U") and not a.startswith("decltype("))
        assert forms.get(owner), (owner, "a launcher or kernel no dispatcher reaches, or a dispatcher with no forms")
        out |= {(kernel, ARMS[kernel][arm], f) for f in forms[owner]}
    assert sites == len(INSTANCE.findall(text)), "an instantiation that is no hipLaunchKernelGGL((k_pg_...<...>) site"
    return out


def _shipped():
    text = ""
    for name in FILES:   # one text: the forms are listed in the header, the sites in the two .hip files
        with open(os.path.join(CSRC, name)) as f:
            text += f.read()
    return instantiations(text)


def _functions(module):
    """Names of the module's top-level functions, from the file (no import)."""
    path = os.path.join(TESTS, module + ".py")
    with open(path) as f:
        return {n.name for n in ast.parse(f.read(), path).body if isinstance(n, ast.FunctionDef)}


def test_the_parser_reduces_a_site_to_kernel_arm_and_form():
    text = """
decltype(auto) with_pg_form(bool vec, const PGView &v, F &&f) {
  return !vec ? f(BoolC<false>{}, IntC<1>{}) : f(BoolC<true>{}, IntC<kPgU>{});
}
static void launch_pg_new(const float *x) {
  if (c) hipLaunchKernelGGL((k_pg_fq_fwd<VEC, U, true, false>), grid, block, 0, st, x);
  else hipLaunchKernelGGL((k_pg_fq_fwd<VEC, U, false, false>), grid, block, 0, st, x);
}
int entry() {
  with_pg_form(vec, v, [&](auto V, auto U) { launch_pg_new<decltype(V)::value, decltype(U)::value>(x); });
  with_bool(vec, [&](auto V) {
    hipLaunchKernelGGL((k_pg_ste_bwd<decltype(V)::value>), pg_grid(v, 1), block, 0, st, g);
  });
}
"""
    assert instantiations(text) == {("k_pg_fq_fwd", "codes only", SCALAR), ("k_pg_fq_fwd", "codes only", VECU),
                                    ("k_pg_fq_fwd", "plain", SCALAR), ("k_pg_fq_fwd", "plain", VECU),
                                    ("k_pg_ste_bwd", "-", SCALAR), ("k_pg_ste_bwd", "-", VECTOR)}
    for broken in (text.replace("hipLaunchKernelGGL((k_pg_ste_bwd<decltype(V)::value>)", "k_pg_ste_bwd<true><<<1, 2>>>("),
                   text.replace("true, false>", "true, maybe>"), text.replace("IntC<kPgU>", "IntC<2>"),
                   text.replace("int entry() {", "int entry() {\n  launch_pg_new<true, 8>(x);")):
        try:
            instantiations(broken)
        except (AssertionError, KeyError):
            continue
        raise AssertionError("a launch the parser cannot place went unnoticed")


def test_every_shipped_instantiation_is_listed():
    shipped = _shipped()
    assert shipped == set(TABLE), {"not listed": sorted(shipped - set(TABLE)), "stale": sorted(set(TABLE) - shipped)}
    forward = [k for k in shipped if k[0] in ("k_pg_observe_fq", "k_pg_fq_fwd")]
    assert len(forward) == 27 and len(shipped) == 27 + 3 + 6 + 10


def test_every_listed_test_exists():
    for key, tests in TABLE.items():
        assert tests, key
        for module, fn in tests:
            assert fn.startswith("test_") and fn in _functions(module), (key, module, fn)
