"""Every solver path of the device on the inputs of tests/solver_special_cases.py -- signed zeros, subnormals, non-finite values, the extremes
of flame_nltgv2_params -- against the CPU checker, compared as BITS (tests/helpers.assert_state_bits_equal: -0.0 is not +0.0, a NaN equals
any NaN).  The solver exists six times over, each form with arithmetic of its own (packed pairs, v_med3_f32 or min / max for the dual's
clamp, compare-and-select clamps, DPP row sums with a neutral element for the lanes that hold nothing); the rest of the suite holds them
to the checker on positive data around 1 only, and with a comparison that takes -0.0 for +0.0.

The paths, forced as tests/test_gpu_parity.py and tests/test_pv_lean.py force them; the path is asserted at the 7-step run (below four
steps the library may go one launch per step -- those runs are compared all the same; the lean kernel, where required, runs them too).
One Regularizer per path takes case after case.  Nothing here injects a fault or withholds a record; after every run of a persistent
form nothing may have been recovered (a run whose wait expired would be redone by another kernel and still match).

tests/test_solver_special_values_ref.py holds the same references against the numpy restatement, and each case to its edge, without a GPU."""
import numpy as np
import pytest

from tests import solver_special_cases as cases
from tests.helpers import ALL_STATE_KEYS, assert_state_bits_equal, float_bits

pytestmark = pytest.mark.gpu

F = np.float32
# name -> (options, last_run_path of a 7-step run, largest degree the path takes, whether it takes graphs whose edges join random pairs)
PATHS = {
    "four kernels": ((("OPT_SOLVER", 1),), 4, 1 << 30, True),
    "fused step": ((("OPT_PERSISTENT", 0),), 2, 1 << 30, True),
    "k_persistent_tv": ((("OPT_PERSISTENT", 3),), 5, 1 << 30, True),
    "k_persistent_pv": ((("OPT_PERSISTENT", 4), ("OPT_PV_LEAN", 1)), 6, 64, True),
    "k_persistent_pv_lean": ((("OPT_PV_LEAN", 2),), 6, 16, True),   # (a vertex of 17 edges is refused: tests/test_pv_lean.py)
    # (a patch of two half-edges per lane fetches at most 64 distinct foreign records: the library runs G, whose edges join random
    #  pairs, one launch per step under this option -- this kernel meets the cases made from G on the local graph L)
    "k_persistent_pv2": ((("OPT_PERSISTENT", 6),), 7, 32, False),
}


def taken(path, case_list):
    return [c for c in case_list if c.max_degree() <= PATHS[path][2] and (c.local or PATHS[path][3])]


@pytest.fixture(scope="module")
def env(built):
    import torch  # noqa: F401  (first: one HIP runtime)

    import flame_amd

    return flame_amd


@pytest.fixture(scope="module")
def regs(env):
    """One context per path, made when first asked for, closed with the module."""
    made = {}

    def get(path):
        if path not in made:
            reg = env.Regularizer(0)
            for name, value in PATHS[path][0]:
                reg.set_option(getattr(env.regularizer, name), value)
            made[path] = reg
        return made[path]

    yield get
    for reg in made.values():
        reg.close()


def params_of(flame_amd, case):
    return flame_amd.Params(**case.params)


def run_case(flame_amd, reg, path, case, n):
    """Uploads the case, runs n steps; returns the state.  Path and recovery are checked here."""
    reg.upload_graph(case.graph())
    reg.run(params_of(flame_amd, case), n)
    info = reg.info()
    assert info["timeouts_recovered"] == 0 and info["torn_records_detected"] == 0, (path, case, n, info["timeouts_recovered"])
    if n >= 7:
        assert info["last_run_path"] == PATHS[path][1], (path, case, n, info["last_run_path"])
    return reg.download_state(ALL_STATE_KEYS)


def compare_cases(flame_amd, reg, path, case_list, after=None):
    """Every case the path takes, every step count of it, all twelve arrays as bits; every difference is collected before the test fails,
    so that one run tells all of them."""
    failures, ran = [], 0
    for case in taken(path, case_list):
        for n in case.steps:
            ref, bad = cases.reference(case, n)
            assert bad == 0, (case, n)
            try:
                out = run_case(flame_amd, reg, path, case, n)
                assert_state_bits_equal(out, ref, what=f"{path}: {case}, {n} steps")
                if after is not None:
                    after(case, n, ref)
            except AssertionError as e:
                failures.append(str(e))
            ran += 1
    assert ran > 0
    assert not failures, f"{len(failures)} of {ran} runs differ:\n" + "\n".join(failures)


def cost_addends(ref):
    """The addends of smoothnessCost and dataCost (cc:51-85) over the state `ref`, formed as the checker forms them."""
    i, j = ref["src"], ref["dst"]
    dx, dy = ref["pos"][i, 0] - ref["pos"][j, 0], ref["pos"][i, 1] - ref["pos"][j, 1]
    a = np.abs(((ref["x"][i] - ref["x"][j]) - ref["w1"][i] * dx) - ref["w2"][i] * dy)
    terms = np.empty(2 * ref["E"], F)
    terms[0::2] = ref["alpha"] * a
    terms[1::2] = ref["beta"] * np.abs(ref["w1"][i] - ref["w1"][j]) + ref["beta"] * np.abs(ref["w2"][i] - ref["w2"][j])
    return terms, np.abs((ref["x"] - ref["data_term"]) * ref["data_weight"]).astype(F)


def bits_of(values):
    return [f"0x{int(b):08X}" for b in float_bits(np.array(values, F))]


@pytest.mark.parametrize("path", list(PATHS))
def test_value_cases_bit_for_bit(env, regs, path):
    """subnormal_all, subnormal_band, negative_zero_data, negative_zero_duals and the seven hubs, 1, 2 and 7 steps.  After the 7-step runs of
    the first three also the costs: the sequential sums equal the checker's, the sums formed on the device (FLAME_NLTGV2_OPT_COST_SUM = 1)
    equal the CPU restatement of their fixed order over the reference's addends -- as float32 bits."""
    from oracle import capi as oracle

    reg = regs(path)
    OPT_COST_SUM = env.regularizer.OPT_COST_SUM

    def costs_too(case, n, ref):
        if n != 7 or case.kind not in ("subnormal_all", "subnormal_band", "negative_zero_data"):
            return
        p = params_of(env, case)
        exact = reg.costs(p)
        reg.set_option(OPT_COST_SUM, 1)
        try:
            fast = reg.costs(p)
        finally:
            reg.set_option(OPT_COST_SUM, 0)
        want = oracle.costs(ref, oracle.make_params(**case.params))
        assert bits_of(exact) == bits_of(want), f"{path}: {case}: costs {exact} against the checker's {want}"
        terms, dterms = cost_addends(ref)
        want_fast = (F(p.data_factor) * F(oracle.strided_tree_sum(terms)), F(oracle.strided_tree_sum(dterms)))
        assert bits_of(fast) == bits_of(want_fast), f"{path}: {case}: costs summed on the device {fast} against {want_fast}"

    compare_cases(env, reg, path, cases.VALUE_CASES, after=costs_too)


@pytest.mark.parametrize("path", list(PATHS))
def test_subnormals_across_xcds_bit_for_bit(env, regs, path):
    """The 320x240 frame under both scalings, 7 steps: its patches sit on all eight XCDs, the subnormal x_bar and w_bar cross them in the
    records.  (That the scaled frame still meets the floors, scaled to its size, is asserted on the checker here as well.)"""
    reg = regs(path)
    failures = []
    for case in cases.FRAME_CASES:
        cases.check_reaches(case, cases.references(case))
        ref, bad = cases.reference(case, 7)
        assert bad == 0
        try:
            assert_state_bits_equal(run_case(env, reg, path, case, 7), ref, what=f"{path}: {case}, 7 steps")
        except AssertionError as e:
            failures.append(str(e))
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("path", list(PATHS))
def test_params_extremes_bit_for_bit(env, regs, path):
    """theta 0 and 1, x_min = x_max, x_min > x_max, data_factor, step_x, step_q 0, infinite and negative bounds; data around 1 and data of
    both signs; 7 steps."""
    compare_cases(env, regs(path), path, cases.PARAM_CASES)


@pytest.mark.parametrize("path", list(PATHS))
def test_non_finite_is_reported_exactly_where_the_checker_reports_it(env, regs, path):
    """FLAME_NLTGV2_ERR_NAN exactly where the checker returns non-zero -- an infinity, an overflow that reaches one, a NaN, at the first,
    the last and an inner vertex -- and a clean run exactly where it returns zero: a NaN datum that no dual has read yet (one step), values
    that are overwritten before they are read, a poisoned vertex without an edge.  Where the run succeeds the state, NaNs included,
    equals the checker's; after an error the context takes G (L for k_persistent_pv2) and two steps and equals the checker again."""
    flame_amd = env
    reg = regs(path)
    ERR_NAN = flame_amd.regularizer.ERR_NAN
    clean = (cases.Case("G after an error", cases.base_graph, "plain", steps=(2,)) if PATHS[path][3] else
             cases.Case("L after an error", cases.local_graph, "plain", steps=(2,)))
    failures, reported, succeeded = [], 0, 0
    for case in taken(path, cases.NON_FINITE_CASES):
        for n in case.steps:
            assert n <= 7
            ref, bad = cases.reference(case, n)
            try:
                reg.upload_graph(case.graph())
                status = 0
                try:
                    reg.run(flame_amd.Params(), n)
                except flame_amd.NLTGV2Error as e:
                    status = e.status
                assert status == (ERR_NAN if bad else 0), f"{path}: {case}, {n} steps: status {status}, the checker reports {bad}"
                info = reg.info()
                assert info["timeouts_recovered"] == 0, (path, case, n)
                if bad:
                    reported += 1
                    out = run_case(flame_amd, reg, path, clean, 2)
                    assert_state_bits_equal(out, cases.reference(clean, 2)[0], what=f"{path}: {clean}, 2 steps after the error of {case}, {n} steps")
                else:
                    succeeded += 1
                    if n >= 7:
                        assert info["last_run_path"] == PATHS[path][1], (path, case, n, info["last_run_path"])
                    assert_state_bits_equal(reg.download_state(ALL_STATE_KEYS), ref, what=f"{path}: {case}, {n} steps")
            except AssertionError as e:
                failures.append(str(e))
    assert not failures, f"{len(failures)} differences:\n" + "\n".join(failures)
    assert reported >= 15 and succeeded >= 12, (reported, succeeded)


@pytest.mark.parametrize("path", list(PATHS))
def test_upload_then_download_returns_the_bits_that_went_in(env, regs, path):
    """No step in between: all twelve arrays of negative_zero_data (every -0.0 of it) and of subnormal_band come back as they went in."""
    reg = regs(path)
    for case in taken(path, [c for c in cases.VALUE_CASES if c.kind in ("negative_zero_data", "subnormal_band")]):
        g = case.graph()
        reg.upload_graph(g)
        assert_state_bits_equal(reg.download_state(ALL_STATE_KEYS), g, what=f"{path}: {case}, upload then download")
