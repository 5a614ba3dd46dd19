"""k_persistent_pv_lean (flame_amd/csrc/nltgv2_persistent_lean.hip): the patch-per-wave kernel's hand-written instance for few
patches per CU.  Every GPU case compares all nine state arrays plus the three prev arrays with the CPU checker bit for bit, with the
lean kernel required (FLAME_NLTGV2_OPT_PV_LEAN = 2: the run fails unless that kernel runs it) and with it off (= 1: the general kernel)
on the same input.  A lean run whose wait expired would be redone by the general kernel and still match, so every required run
also checks that nothing was recovered.  One test needs no GPU: the register counts of the kernel as built against its residency
function."""
import os
import re
import subprocess

import numpy as np
import pytest

from flame_amd import synth
from tests.conftest import ROOT
from tests.helpers import OUT_KEYS, assert_state_equal, random_graph

ALL_KEYS = OUT_KEYS + ("x_prev", "w1_prev", "w2_prev")
LEAN_SRC = os.path.join(ROOT, "flame_amd", "csrc", "nltgv2_persistent_lean.hip")


@pytest.fixture(scope="module")
def env(built):
    import torch  # noqa: F401  (first: one HIP runtime)

    import flame_amd
    from oracle import capi as oracle

    return flame_amd, oracle


def cpu_run(oracle, g, n, **pkw):
    ref = synth.copy_graph(g)
    assert oracle.run(ref, n, oracle.make_params(**pkw)) == 0
    return ref


def both_kernels(flame_amd, g, n, ref, what, params=None):
    """The same input through the lean kernel (required) and through the general one: both equal the checker's state."""
    from flame_amd.regularizer import OPT_PV_LEAN

    for lean in (2, 1):
        with flame_amd.Regularizer(0) as reg:
            reg.set_option(OPT_PV_LEAN, lean)
            reg.upload_graph(g)
            reg.run(params or flame_amd.Params(), n)
            info = reg.info()
            if lean == 2:
                assert info["last_run_path"] == 6 and info["timeouts_recovered"] == 0, (what, info["last_run_path"], info["timeouts_recovered"])
            assert_state_equal(reg.download_state(), ref, keys=ALL_KEYS, what=f"{what}, PV_LEAN={lean}, {n} steps")


_GRAPHS = {}


def config_graph(config):
    if config not in _GRAPHS:
        _GRAPHS[config] = synth.make_graph(config, seed=7)
    return _GRAPHS[config]


def with_hubs(g0, hub_degrees, seed):
    """g0 plus edges that bring one vertex each to the degrees asked for, the edge list shuffled: the
    accumulation order of a hub (ascending edge id) is spread over the list."""
    rng = np.random.default_rng(seed)
    V = g0["V"]
    edges = [tuple(e) for e in np.stack([g0["src"], g0["dst"]], 1)]
    deg = np.bincount(np.concatenate([g0["src"], g0["dst"]]), minlength=V)
    hubs = rng.choice(np.flatnonzero(deg <= min(hub_degrees)), len(hub_degrees), replace=False)
    for h, want in zip(hubs, hub_degrees):
        have = {b if a == h else a for a, b in edges if h in (a, b)}
        cands = [v for v in rng.permutation(V) if v != h and v not in have and v not in hubs and deg[v] < 8]
        for v in cands[: max(0, want - len(have))]:
            edges.append((h, v) if rng.random() < 0.5 else (v, h))
            deg[v] += 1
        deg[h] = max(want, len(have))
    e = np.array(edges, np.int32)[rng.permutation(len(edges))]
    g = synth.assemble_graph(g0["pos"], g0["data_term"], e)
    got = np.bincount(np.concatenate([g["src"], g["dst"]]), minlength=V)
    assert sorted(got[hubs]) == sorted(hub_degrees), (got[hubs], hub_degrees)
    return g, got


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 2, 7, 200])
@pytest.mark.parametrize("config", ["320x240", "640x480"])
def test_frames_for_odd_and_even_step_counts(env, config, n):
    """A single frame on all eight XCDs with placed records; 1, 2, 7, 200 steps: the two-step loop, its tail, and neither."""
    flame_amd, oracle = env
    g = config_graph(config)
    both_kernels(flame_amd, g, n, cpu_run(oracle, g, n), config)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 8, 31])
def test_a_graph_small_enough_for_one_xcd(env, n):
    """At most two patches per CU of one XCD: the launch stays there, no placed records, no rotation of the grid."""
    flame_amd, oracle = env
    g = random_graph(420, 1200, seed=11)
    assert np.bincount(np.concatenate([g["src"], g["dst"]])).max() <= 16
    both_kernels(flame_amd, g, n, cpu_run(oracle, g, n), "one XCD")


def grid_with_one_hub(degree, seed):
    """A jittered 40x30 grid with right, down and one diagonal edge (largest degree 6) plus ONE hub brought to `degree` by edges to
    vertices that stay below 8: whatever patch holds the hub, `degree` is that patch's largest, so the exit it selects is the one taken."""
    rng = np.random.default_rng(seed)
    W, H = 40, 30
    V = W * H
    ii, jj = np.meshgrid(np.arange(W), np.arange(H))
    pos = (np.stack([ii.ravel(), jj.ravel()], 1) * 8.0 + rng.random((V, 2)) * 3.0).astype(np.float32)
    data = (0.5 + rng.random(V)).astype(np.float32)
    vid = lambda x, y: y * W + x  # noqa: E731
    edges = []
    for y in range(H):
        for x in range(W):
            if x + 1 < W:
                edges.append((vid(x, y), vid(x + 1, y)))
            if y + 1 < H:
                edges.append((vid(x, y + 1), vid(x, y)))
            if x + 1 < W and y + 1 < H:
                edges.append((vid(x, y), vid(x + 1, y + 1)))
    hub = vid(W // 2, H // 2)
    have = {b if a == hub else a for a, b in edges if hub in (a, b)}
    assert len(have) == 6
    far = [v for v in rng.permutation(V) if v != hub and v not in have][: degree - 6]
    edges += [(hub, v) if k % 2 else (v, hub) for k, v in enumerate(far)]
    e = np.array(edges, np.int32)[rng.permutation(len(edges))]  # the hub's edges spread over the list: the accumulation order
    g = synth.assemble_graph(pos, data, e)
    deg = np.bincount(np.concatenate([g["src"], g["dst"]]), minlength=V)
    assert deg[hub] == degree and np.delete(deg, hub).max() <= 7
    return g


@pytest.mark.gpu
def test_every_exit_of_the_larger_degrees(env):
    """The code behind the common path leaves at a patch's largest degree of 10, 12, 13, 14 or 16.  One hub per graph, nobody else
    above 7 edges: the hub's patch has exactly that largest degree (9, 11 and 15 run into the next exit), odd and even step counts."""
    flame_amd, oracle = env
    for degree in (9, 10, 11, 12, 13, 14, 15, 16):
        g = grid_with_one_hub(degree, seed=degree)
        for n in (2, 9):
            both_kernels(flame_amd, g, n, cpu_run(oracle, g, n), f"one hub of {degree} edges")


@pytest.mark.gpu
def test_a_vertex_of_seventeen_edges_is_the_general_kernels(env):
    """The lean kernel takes graphs of largest degree 16 at most: a 17-edge star runs the general kernel by default, and where the
    lean kernel is required the run fails cleanly -- nothing ran, the context goes on."""
    flame_amd, oracle = env
    from flame_amd.regularizer import OPT_PV_LEAN

    g, deg = with_hubs(synth.make_graph("320x240", seed=44), (17,), seed=6)
    assert deg.max() == 17
    ref = cpu_run(oracle, g, 9)
    with flame_amd.Regularizer(0) as reg:
        reg.set_option(OPT_PV_LEAN, 2)
        reg.upload_graph(g)
        with pytest.raises(flame_amd.NLTGV2Error) as ei:
            reg.run(flame_amd.Params(), 9)
        assert ei.value.status == -1  # FLAME_NLTGV2_ERR_INVALID_ARG
        assert_state_equal(reg.download_state(), g, keys=ALL_KEYS, what="after the refused run: the initial state")
        reg.set_option(OPT_PV_LEAN, 0)
        reg.run(flame_amd.Params(), 9)
        assert reg.info()["last_run_path"] == 6
        assert_state_equal(reg.download_state(), ref, keys=ALL_KEYS, what="17-edge star, general kernel")


@pytest.mark.gpu
def test_isolated_vertex_and_a_component_of_one_patch(env):
    """A vertex without an edge (its head adds nothing to its own state) and components that fit one patch: no fetch list, every
    neighbour in LDS."""
    flame_amd, oracle = env
    rng = np.random.default_rng(3)
    pos = (rng.random((9, 2)) * 20).astype(np.float32)
    data = (0.5 + rng.random(9)).astype(np.float32)
    edges = np.array([(0, 1), (2, 1), (2, 3), (3, 0), (0, 2), (5, 6), (7, 6)], np.int32)  # vertex 4 and vertex 8: no edge
    g = synth.assemble_graph(pos, data, edges)
    for n in (1, 6):
        both_kernels(flame_amd, g, n, cpu_run(oracle, g, n), "isolated vertex, one patch")
    g1 = synth.assemble_graph(pos[:1], data[:1], np.zeros((0, 2), np.int32))
    both_kernels(flame_amd, g1, 5, cpu_run(oracle, g1, 5), "a single vertex")


@pytest.mark.gpu
def test_both_clamps_and_all_three_prox_branches(env):
    """Non-default parameters: x_min and x_max inside the data's range (both compare-and-select clamps fire), a threshold small
    enough for both shifted branches of proxL1 and large enough for the middle one, theta away from its default."""
    flame_amd, oracle = env
    g = synth.make_graph("320x240", seed=9)
    rng = np.random.default_rng(9)
    g["data_term"] = (0.5 + rng.random(g["V"])).astype(np.float32)
    g["x"] = g["data_term"].copy(); g["x_bar"] = g["data_term"].copy(); g["x_prev"] = g["data_term"].copy()
    g["data_weight"] = (0.2 + 3.0 * rng.random(g["V"])).astype(np.float32)
    kw = dict(data_factor=0.37, step_x=0.004, step_q=31.0, theta=0.6, x_min=0.7, x_max=1.3)
    n = 41
    ref = cpu_run(oracle, g, n, **kw)
    x, d = ref["x"], ref["data_term"]
    inside = (x > np.float32(0.7)) & (x < np.float32(1.3))
    assert (x == np.float32(0.7)).any() and (x == np.float32(1.3)).any(), "both clamps"
    # the last step's branch by its result: x below the data = shifted up, above = shifted down, equal = the middle branch
    assert (inside & (x < d)).any() and (inside & (x > d)).any() and (inside & (x == d)).any(), "all three proxL1 branches"
    both_kernels(flame_amd, g, n, ref, "non-default params", params=flame_amd.Params(**kw))


@pytest.mark.gpu
def test_two_frame_union_below_the_pacing_bound(env):
    flame_amd, oracle = env
    frames = [config_graph("640x480"), synth.make_graph("640x480", seed=8)]
    union = synth.concat_graphs(frames)
    n = 12
    refs = [cpu_run(oracle, f, n) for f in frames]
    ref = {k: np.concatenate([r[k] for r in refs]) for k in ALL_KEYS}
    both_kernels(flame_amd, union, n, ref, "two frames of 640x480")


@pytest.mark.gpu
def test_three_run_async_calls_then_sync(env):
    """Back-to-back asynchronous runs chain onto each other unchecked: three lean launches, one check at the end."""
    flame_amd, oracle = env
    from flame_amd.regularizer import OPT_PV_LEAN

    g = config_graph("320x240")
    ref = synth.copy_graph(g)
    for n in (7, 10, 5):
        assert oracle.run(ref, n, oracle.make_params()) == 0
    for lean in (2, 1):
        with flame_amd.Regularizer(0) as reg:
            reg.set_option(OPT_PV_LEAN, lean)
            reg.upload_graph(g)
            for n in (7, 10, 5):
                reg.run_async(flame_amd.Params(), n)
            reg.sync()
            info = reg.info()
            assert info["last_run_path"] == 6 and info["timeouts_recovered"] == 0
            assert_state_equal(reg.download_state(), ref, keys=ALL_KEYS, what=f"chain of three, PV_LEAN={lean}")


def test_lean_kernel_registers_match_its_residency_function(tmp_path):
    """pv_lean_real_waves_per_simd (nltgv2_persistent_lean.hip) is derived from the register counts of the kernel as built, by the
    rule of tests/test_abi.py: waves per SIMD = min(512 // VGPRs rounded up to 8, 800 // (SGPRs rounded up to 16, + 16), 8).  The
    kernel must not use scratch: a spill reload would sit in the hand-off path or in front of a wait."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math",
           "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "flame_amd", "csrc"), "-c", LEAN_SRC, "-o", str(tmp_path / "k.o"),
           "-Rpass-analysis=kernel-resource-usage"]
    rep = subprocess.run(cmd, capture_output=True, text=True, check=True).stderr
    found = {}
    for m in re.finditer(r"Function Name: (\S+).*?TotalSGPRs: (\d+).*?VGPRs: (\d+).*?ScratchSize \[bytes/lane\]: (\d+)", rep, flags=re.S):
        if "k_persistent_pv_lean" in m.group(1):
            found[m.group(1)] = (int(m.group(2)), int(m.group(3)), int(m.group(4)))
    assert len(found) == 1, sorted(found)
    sg, vg, scratch = next(iter(found.values()))
    assert scratch == 0
    assume = re.search(r"int pv_lean_real_waves_per_simd\(\) \{.*?return (\d+);", open(LEAN_SRC).read(), flags=re.S)
    assert assume, "the residency function of the lean kernel"
    real = min(512 // ((vg + 7) // 8 * 8), 800 // ((sg + 15) // 16 * 16 + 16), 8)
    assert real >= int(assume.group(1)), f"{vg} VGPRs / {sg} SGPRs keep {real} waves per SIMD, the planner assumes {assume.group(1)}"
    assert 4 * int(assume.group(1)) >= 13, "the regime the kernel runs in has up to kPvPaceAbovePerCu = 13 patches per CU"
