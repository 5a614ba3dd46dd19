"""The reference side of tests/test_gpu_solver_special_values.py, without a GPU: for every case of tests/solver_special_cases.py and every
step count the device is held to, the C checker (oracle/nltgv2_oracle.c) and the independently written numpy restatement
(oracle/nltgv2_numpy.py) agree bit for bit -- signed zeros and subnormals included, a NaN equal to any NaN -- and on whether a NaN dual
was reported; every case still reaches the edge it is there for (check_reaches); and the bit-level comparison itself tells what it
must tell."""
import numpy as np
import pytest

from flame_amd import synth
from oracle import capi as oracle
from oracle import nltgv2_numpy
from tests import solver_special_cases as cases
from tests.helpers import ALL_STATE_KEYS, OUT_KEYS, assert_state_bits_equal, assert_state_equal

F = np.float32


@pytest.mark.parametrize("case", cases.ALL_CASES, ids=repr)
def test_checker_and_numpy_restatement_agree_bit_for_bit(built, case):  # (built: the frame cases triangulate with the library)
    params = dict(oracle.DEFAULT_PARAMS, **case.params)
    for n in case.steps:
        ref, bad = cases.reference(case, n)
        other = synth.copy_graph(case.graph())
        with np.errstate(all="ignore"):  # (inf - inf, inf / inf and 0 * inf are what some of these cases are about)
            other_bad = nltgv2_numpy.run(other, n, params)
        assert int(other_bad) == bad, (case, n, bad, other_bad)
        assert_state_bits_equal(ref, other, what=f"{case}, {n} steps, C against numpy")


@pytest.mark.parametrize("case", cases.ALL_CASES, ids=repr)
def test_every_case_reaches_its_edge(built, case):
    cases.check_reaches(case, cases.references(case))


def test_a_case_that_lost_its_edge_fails():
    """check_reaches is not vacuous: the plain graph G in the place of a case's input meets none of the floors."""
    for kind in ("subnormal_all", "subnormal_band", "negative_zero_data", "negative_zero_duals"):
        plain = cases.Case(f"plain G as {kind}", cases.base_graph, kind)
        with pytest.raises(AssertionError):
            cases.check_reaches(plain, cases.references(plain))

    def hub_from_plus_zero():
        g = cases.negative_zero_hub(9)
        for k in cases.W_KEYS:
            g[k][:] = F(0.0)
        return g

    hub = cases.Case("a hub whose w start at +0.0", hub_from_plus_zero, "negative_zero_hub", arg=9)
    with pytest.raises(AssertionError):
        cases.check_reaches(hub, cases.references(hub))
    clean = cases.Case("non-finite: nothing poisoned", cases.base_graph_with_an_isolated_vertex, "non_finite", arg=1)
    with pytest.raises(AssertionError):
        cases.check_reaches(clean, cases.references(clean))


def test_the_inputs_are_what_the_recipes_say(built):
    g = cases.base_graph()
    deg = cases.degrees(g)
    assert g["V"] == 420 and g["E"] == 1200 and deg.max() <= 16
    iso = cases.base_graph_with_an_isolated_vertex()
    assert cases.degrees(iso)[cases.ISOLATED] == 0 and cases.degrees(iso).max() <= 16 and cases.LAST == iso["V"] - 1
    assert cases.degrees(iso)[[0, 17, 18, cases.LAST]].min() > 0, "the poisoned vertices that must report have edges"
    for d in cases.HUB_DEGREES:
        h = cases.negative_zero_hub(d)
        assert h["V"] == 61 + d and cases.degrees(h)[0] == d and cases.degrees(h).max() == max(d, 3)
        spokes = h["src"] == 0
        assert spokes.sum() == d and not (h["dst"] == 0).any()
        assert np.all(h["pos"][0] == 0) and np.all(h["pos"][1:] > 0)  # dx < 0 and dy < 0 along every edge of the hub
        assert len(set(np.flatnonzero(spokes))) == d and np.flatnonzero(spokes).max() - np.flatnonzero(spokes).min() >= d, "the hub's edges are spread over the list"
    loc = cases.local_graph()
    assert loc["V"] == 420 and np.array_equal(loc["data_term"], g["data_term"]) and np.array_equal(loc["data_weight"], g["data_weight"])
    assert abs(float(np.median(loc["alpha"])) / float(np.median(g["alpha"])) - 1.0) < 0.5, "L's edges are about as long as G's"
    iso_l = cases.with_an_isolated_vertex(cases.local_graph())
    assert cases.degrees(iso_l)[cases.ISOLATED] == 0 and cases.degrees(iso_l)[[0, 5, 17, 18, cases.LAST]].min() > 0
    frame = cases.FRAME_CASES[0].graph()
    assert frame["V"] == 2120 and cases.degrees(frame).max() <= 16
    # every case made from G stands on L as well (the graph k_persistent_pv2 takes), the hubs and the frames are local as they are
    for group in (cases.VALUE_CASES, cases.PARAM_CASES, cases.NON_FINITE_CASES):
        assert {c.name + " on L" for c in group if not c.local} == {c.name for c in group if c.name.endswith(" on L")}


# ---- assert_state_bits_equal itself -------------------------------------------------------------------------------------------
def _state(**over):
    s = {k: np.linspace(0.5, 1.5, 7).astype(F) for k in ALL_STATE_KEYS}
    s.update({k: np.asarray(v, F) for k, v in over.items()})
    return s


def test_bit_comparison_tells_the_zeros_apart():
    a, b = _state(), _state()
    a["w1"][3], b["w1"][3] = F(-0.0), F(0.0)
    assert_state_equal(a, b, keys=ALL_STATE_KEYS)  # the value comparison passes ...
    with pytest.raises(AssertionError) as ei:
        assert_state_bits_equal(a, b, what="zeros")
    msg = str(ei.value)
    assert "zeros" in msg and "w1" in msg and "[3]" in msg and "0x80000000" in msg and "0x00000000" in msg, msg


def test_bit_comparison_fails_on_one_ulp_and_names_the_first_difference():
    a, b = _state(), _state()
    b["q2"][5] = np.nextafter(a["q2"][5], F(2))
    b["q2"][6] = F(9)
    with pytest.raises(AssertionError) as ei:
        assert_state_bits_equal(a, b, what="ulp")
    msg = str(ei.value)
    bits = lambda v: f"0x{int(np.asarray(v, F).view(np.uint32)):08X}"  # noqa: E731
    assert "q2" in msg and "[5]" in msg and bits(a["q2"][5]) in msg and bits(b["q2"][5]) in msg and "2/7" in msg, msg
    sub = _state(x=[0, 0, 0, 0, 0, 0, 1e-45])  # the smallest subnormal against zero
    with pytest.raises(AssertionError):
        assert_state_bits_equal(sub, _state(x=[0] * 7))
    assert_state_bits_equal(a, b, keys=OUT_KEYS[:3])  # only the keys asked for are compared


def test_bit_comparison_takes_any_nan_for_any_nan_and_nothing_else():
    x86 = np.array([0xFFC00000, 0x3F800000], np.uint32).view(F)     # what x86 generates for inf - inf
    gfx = np.array([0x7FC00000, 0x3F800000], np.uint32).view(F)     # what gfx950 generates
    payload = np.array([0x7FC12345, 0x3F800000], np.uint32).view(F)
    keys = ("x",)
    assert_state_bits_equal({"x": x86}, {"x": gfx}, keys=keys)
    assert_state_bits_equal({"x": payload}, {"x": gfx}, keys=keys)
    with pytest.raises(AssertionError):
        assert_state_bits_equal({"x": x86}, {"x": np.array([np.inf, 1], F)}, keys=keys)
    with pytest.raises(AssertionError):
        assert_state_bits_equal({"x": np.array([np.inf, 1], F)}, {"x": np.array([-np.inf, 1], F)}, keys=keys)
    with pytest.raises(AssertionError):
        assert_state_bits_equal({"x": x86}, {"x": x86[:1]}, keys=keys)
    assert x86.view(np.uint32)[0] == 0xFFC00000, "the comparison leaves its inputs alone"
