"""The device topology builder (flame_amd/csrc/nltgv2_topo.hip, nltgv2_topo_capi.hip) on graphs that are not one Delaunay frame:
paths, forests of tiny components, hubs at every threshold of walk_place, vertex counts at the builder's granularities,
degenerate positions, colliding and returning feature ids, and the corners of the sync front (tests/topology_cases.py).

The CPU tests pin the generators: a family built to have a property is checked for it, so that a GPU test cannot go vacuous.
The GPU tests prove that the DEVICE builder made the tables through the sync route: a two-vertex seed graph whose ids the case does
not use, FLAME_NLTGV2_OPT_SYNC_PATH = 2 (device or error), sync_graph(..., edges_unique=True) -- every vertex is new, the builder
builds the whole topology.  Then, in this order: last_sync_path == 2; the device tables word for word the host builders'
(flame_nltgv2_layout_selftest); the edge list the syncGraph restatement's (oracle/sync_oracle.py); after runs of an odd and an even
length in the persistent forms 4, 3 (and 6 up to 32 edges per vertex) all nine state arrays and the three prev arrays the
checker's, exactly.  Everything is integer tables and bit-identical floats: no tolerance anywhere."""
import numpy as np
import pytest

from flame_amd import synth
from oracle import capi as oracle
from oracle import sync_oracle
from tests import topology_cases as tc
from tests.helpers import OUT_KEYS, assert_state_equal

ALL_KEYS = OUT_KEYS + ("x_prev", "w1_prev", "w2_prev")
RUNS = (7, 20)  # one odd, one even


_CASES = {}


def case(name):
    """(pos, data, edges, note) of a named case, made once."""
    if name not in _CASES:
        if name == "path":
            c = tc.path(1300)
        elif name == "forest":
            c = tc.forest(700)
        elif name == "forest+grid":
            c = tc.forest(400, with_grid=True)
        elif name == "collinear":
            c = tc.collinear(700)
        elif name == "stacked":
            c = tc.stacked()
        elif name == "hubs":
            c = tc.grid_with_hubs(tc.HUB_DEGREES)
        elif name == "hub65":
            c = tc.grid_with_hubs((65,))
        else:
            c = tc.sized(int(name.split("-")[1]))
        _CASES[name] = c
    return _CASES[name]


SHAPES = ["path", "forest", "forest+grid", "collinear", "stacked", "hubs"] + [f"sized-{v}" for v in tc.SIZED_V]


def walk_borders(pos, edges):
    """Component borders per 512-window of the HOST's walk, and the component label of every walk position: flame_nltgv2_pack_probe
    gives perm, the walk after the degree sort inside a window -- which never moves a vertex across a component border, so the
    components stand in perm exactly where they stand in order_m."""
    from flame_amd import regularizer

    V = len(pos)
    g = dict(V=V, E=len(edges), pos=pos, src=np.ascontiguousarray(edges[:, 0]), dst=np.ascontiguousarray(edges[:, 1]))
    perm = regularizer.pack_probe(g)["perm"][:V]
    label = tc.components(V, edges)[perm]
    border = np.concatenate([[True], label[1:] != label[:-1]])
    per_window = [int(border[w:w + 512].sum()) for w in range(0, V, 512)]
    return per_window, label


def restated(name, n=20):
    """The case synced into the seed graph by the restatement, then n steps of the checker -> (flat graph, NaN count)."""
    pos, data, edges, _ = case(name)
    fid = tc.case_ids(len(pos), 0)
    ref = sync_oracle.RefGraph.from_flat(tc.seed_graph(), tc.SEED_IDS)
    sync_oracle.sync(ref, fid, pos, data, np.ones(len(pos), np.float32), edges)
    flat = sync_oracle.flatten(ref, fid)
    return flat, oracle.run(flat, n)


# ---- CPU: the generators have the properties the GPU tests rely on -------------------------------------------------------------------------
@pytest.mark.parametrize("name", SHAPES + ["hub65"])
def test_generators_are_simple_graphs_the_restatement_and_the_checker_handle(name):
    """Every family: edges in range, no self-loop, no pair twice, no edge between equal positions (alpha = 1 / length would be inf),
    mixed orientation; synced into the two-vertex seed graph by the restatement and run 20 steps by the checker: no NaN."""
    pos, data, edges, note = case(name)
    V = len(pos)
    assert pos.dtype == np.float32 and data.dtype == np.float32 and edges.dtype == np.int32 and data.shape == (V,), note
    assert edges.min() >= 0 and edges.max() < V and np.all(edges[:, 0] != edges[:, 1]), note
    key = np.minimum(edges[:, 0], edges[:, 1]).astype(np.int64) * V + np.maximum(edges[:, 0], edges[:, 1])
    assert len(np.unique(key)) == len(edges), f"{note}: a pair twice"
    assert not np.any(np.all(pos[edges[:, 0]] == pos[edges[:, 1]], axis=1)), f"{note}: an edge of length 0"
    if len(edges) > 8:
        up = int((edges[:, 0] < edges[:, 1]).sum())
        assert 0 < up < len(edges), f"{note}: one orientation only"
    assert not set(tc.case_ids(V, 0).tolist()) & set(tc.SEED_IDS.tolist())
    flat, nan_count = restated(name)
    assert nan_count == 0 and (flat["V"], flat["E"]) == (V, len(edges))
    assert all(np.all(np.isfinite(flat[k])) for k in ALL_KEYS), note


def test_path_is_one_path():
    """path(1300): exactly the edges (i, i + 1), one component, two ends -- the chain k_topo_rows / k_topo_hook_min / k_topo_hook have to
    join is as long as the graph."""
    pos, _, edges, _ = case("path")
    deg = tc.degrees(len(pos), edges)
    assert len(pos) == 1300 and len(edges) == 1299 and np.bincount(deg).tolist() == [0, 2, 1298]
    assert len(np.unique(tc.components(len(pos), edges))) == 1
    assert {tuple(e) for e in np.sort(edges, axis=1).tolist()} == {(i, i + 1) for i in range(1299)}


def test_forest_has_hundreds_of_component_borders_in_one_window(built):
    """700 components of 1, 1, 2, 2, 3, 5 vertices; the densest 512-window of the host's own walk holds more than 255 borders (the
    run field of k_topo_windows' sort key needs its ninth bit); isolated vertices stand between connected ones."""
    pos, _, edges, _ = case("forest")
    V = len(pos)
    label = tc.components(V, edges)
    sizes = np.bincount(np.bincount(label, minlength=V))
    assert V == 1630 and len(edges) == 1046
    assert (sizes[1], sizes[2], sizes[3], sizes[5]) == (234, 234, 116, 116) and sizes[1:].sum() == 700
    per_window, walk_label = walk_borders(pos, edges)
    assert max(per_window) > 255, per_window
    size_at = np.bincount(label, minlength=V)[walk_label]
    assert np.any((size_at[1:-1] == 1) & (size_at[:-2] > 1) & (size_at[2:] > 1)), "an isolated vertex between connected ones"


def test_forest_with_grid_has_a_segment_and_a_window_begin_inside_a_component(built):
    """The 30 x 20 grid component covers walk positions 255..256 and 511..512: segment 1 of k_topo_walk and window 1 of k_topo_windows
    begin inside it (no border flag at their first position)."""
    pos, _, edges, _ = case("forest+grid")
    V = len(pos)
    label = tc.components(V, edges)
    counts = np.bincount(label, minlength=V)
    grid = int(np.argmax(counts))
    assert counts[grid] == 600 and len(np.unique(label)) == 401
    _, walk_label = walk_borders(pos, edges)
    assert walk_label[255] == walk_label[256] == grid and walk_label[511] == walk_label[512] == grid
    assert tc.degrees(V, edges).max() == 4


@pytest.mark.parametrize("hub_degrees", [tc.HUB_DEGREES, (65,)])
def test_hub_grids_have_exactly_the_degrees_asked_for(hub_degrees):
    """One hub at each side of every threshold of walk_place -- 8|9 (a row of its own), 16|17 (a patch of its own), 32|33, 48|49
    (two, three, four whole rows), 63, 64|65 (built or declined) --, which are also the thresholds (d + 1) >> 1 = 8|9 and 16|17 of
    the two-half-edges walk at 16|17 and 32|33; everybody else below 8."""
    pos, _, edges, _ = case("hubs" if len(hub_degrees) > 1 else "hub65")
    deg = np.sort(tc.degrees(len(pos), edges))
    assert len(pos) == 1200 and deg[-len(hub_degrees):].tolist() == sorted(hub_degrees) and deg[-len(hub_degrees) - 1] < 8


def test_sized_collinear_and_stacked_have_their_sizes_and_positions():
    """sized(V): exactly V vertices and at least one edge (topo_prepare takes V >= 2, E >= 1) at every granularity of the builder;
    collinear: one y, x strictly increasing (sy == 0 in topo_prepare); stacked: a quarter of the vertices exactly on another vertex of
    the same component (equal WalkKey: the stable radix sort decides)."""
    for V in tc.SIZED_V:
        pos, _, edges, _ = case(f"sized-{V}")
        assert len(pos) == V and len(edges) >= 1, V
    pos, _, edges, _ = case("collinear")
    assert np.all(pos[:, 1] == pos[0, 1]) and np.all(np.diff(pos[:, 0]) > 0) and len(edges) == 2 * len(pos) - 3
    pos, _, edges, _ = case("stacked")
    V = len(pos)
    _, inverse, counts = np.unique(pos, axis=0, return_inverse=True, return_counts=True)
    shared = counts[inverse.reshape(-1)] == 2
    assert counts.max() == 2 and shared.sum() == 2 * (V // 4), "a quarter of the vertices lie on another vertex"
    assert len(np.unique(tc.components(V, edges))) == 1  # (equal Morton codes inside ONE component: the sort's stability decides)


def test_colliding_ids_collide():
    """Restates feat_slot of nltgv2_topo.hip: half of the ids in the last three slots of a 2^12 table, the other half in slot 2048."""
    ids = tc.colliding_ids(480)
    assert len(np.unique(ids)) == 480 and ids.min() >= 0
    slot = ((ids.astype(np.int64) * 0x9E3779B1) % (1 << 32)) >> 20
    assert np.all(slot[:240] >= 4093) and np.all(slot[240:] == 2048)
    assert all((slot[:240] == s).sum() > 2 for s in (4093, 4094, 4095)), "every one of the last three slots holds a chain that wraps"
    assert 2197 == int((tc.feat_slot(np.arange(3_000_000), 12) >= 4093).sum())


# ---- GPU ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def env(built):
    import torch  # noqa: F401  (first: one HIP runtime)

    import flame_amd

    return flame_amd


class Frames:
    """One context and the restatement side by side: sync a frame into both, then make the assertions of the module docstring."""

    def __init__(self, flame_amd, sync_path=2):
        from flame_amd.regularizer import OPT_SYNC_PATH

        self.fa = flame_amd
        self.reg = flame_amd.Regularizer(0)
        g = tc.seed_graph()
        self.reg.upload_graph(g)
        self.reg.set_feature_ids(tc.SEED_IDS)
        self.reg.set_option(OPT_SYNC_PATH, sync_path)
        self.ref = sync_oracle.RefGraph.from_flat(g, tc.SEED_IDS)
        self.fid = tc.SEED_IDS
        self.params = flame_amd.Params()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.reg.close()

    def sync_path(self, value):
        from flame_amd.regularizer import OPT_SYNC_PATH

        self.reg.set_option(OPT_SYNC_PATH, value)

    def sync(self, fid, pos, data, edges, edges_unique=True):
        """The frame into the context and into the restatement."""
        weight = np.ones(len(fid), np.float32)
        self.reg.sync_graph(fid, pos, data, weight, edges, edges_unique=edges_unique)
        sync_oracle.sync(self.ref, fid, pos, data, weight, edges)
        self.fid = np.asarray(fid, np.int32)

    def flat(self):
        return sync_oracle.flatten(self.ref, self.fid)

    def check_graph(self, what, path=2):
        """last_sync_path, selftest, edge list, state as it stands -- in this order."""
        reg = self.reg
        assert reg.info()["last_sync_path"] == path, f"{what}: sync path"
        assert reg.layout_selftest() == 0, f"{what}: device tables differ from the host builders'"
        flat = self.flat()
        src, dst, fid = reg.topology()
        assert np.array_equal(fid, self.fid), f"{what}: feature ids"
        assert np.array_equal(src, flat["src"]) and np.array_equal(dst, flat["dst"]), f"{what}: edge list"
        assert_state_equal(reg.download_state(), flat, keys=ALL_KEYS, what=f"{what}: state after the sync")
        return flat

    def run_forms(self, what, forms=None, runs=RUNS):
        """run(p, n) for an odd and an even n in every persistent form: all twelve arrays equal the checker's on the restatement's graph."""
        from flame_amd.regularizer import OPT_PERSISTENT

        reg = self.reg
        flat = self.flat()
        if forms is None:
            forms = (4, 3) + ((6,) if reg.info()["max_degree"] <= 32 else ())
        for form in forms:
            reg.set_option(OPT_PERSISTENT, form)
            for n in runs:
                reg.run(self.params, n)
                if form in (4, 3) and reg.info()["max_degree"] <= 64:  # (the form asked for ran on these tables, not the per-step sweep)
                    assert reg.info()["last_run_path"] == {4: 6, 3: 5}[form], f"{what}: form {form} ran as path {reg.info()['last_run_path']}"
                assert oracle.run(flat, n) == 0
                assert_state_equal(reg.download_state(), flat, keys=ALL_KEYS, what=f"{what}: form {form}, {n} steps")
        reg.set_option(OPT_PERSISTENT, 1)
        sync_oracle.absorb(self.ref, flat, self.fid)

    def check(self, what, path=2, forms=None):
        self.check_graph(what, path)
        self.run_forms(what, forms)


@pytest.mark.gpu
@pytest.mark.parametrize("name", SHAPES)
def test_shapes_built_on_the_device(env, name):
    """Every kernel of the builder on a shape the Delaunay frames never give it.
    path: k_topo_rows' smallest-neighbour round leaves ~V/3 trees on a chain, k_topo_hook_min / k_topo_hook must join them all.
    forest: k_topo_roots' atomic minimum per (wave, root) with dozens of roots per wave; more than 255 borders in one window
    (k_topo_windows: `run << 16`); patches that end at every border (walk_place's force_new); isolated vertices (degree 0, need 1).
    forest+grid: segment 1 of k_topo_walk and window 1 of k_topo_windows begin inside a component.
    collinear: sy == 0, the Morton code is x alone.  stacked: equal sort keys, the radix sort's stability decides order_m.
    hubs: walk_place at need = 8|9, 16|17, 32|33, 48|49, 63, 64 and (d + 1) >> 1 of them; k_topo_rows' insertion sort of rows up to 64.
    sized-V: V = 2, 3 (cc_bits 1, 2: cc_mix on one and two bits), 64, 256, 512, 1024 and their neighbours (the padding lanes of the
    last slice, the last segment of k_topo_walk, the last-workgroup scan of k_topo_windows over 1, 2, 3 windows)."""
    pos, data, edges, note = case(name)
    with Frames(env) as fr:
        fr.sync(tc.case_ids(len(pos), 0), pos, data, edges)
        fr.check_graph(note)
        if name == "hubs":
            assert fr.reg.info()["max_degree"] == 64
        fr.run_forms(note)


def _must_drop(name, pos, edges):
    V = len(pos)
    if name == "hubs":
        return [int(np.flatnonzero(tc.degrees(V, edges) == 33)[0])]  # one hub goes
    if name == "forest":
        label = tc.components(V, edges)
        return np.flatnonzero(np.isin(label, np.unique(label)[5:60])).tolist()  # whole small components go
    return []


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["forest", "hubs", "sized-512"])
def test_second_frame_on_the_same_context(env, name):
    """The sync front proper (k_topo_init's look-up and insert, k_topo_edges, the scan, k_topo_new_edges) on these shapes: a second
    frame drops ~15 % of the vertices (whole small components, one hub), permutes the caller's vertex order, reverses half of the
    edges, drops and adds pairs between survivors and adds new vertices.  Survivors keep state, edge duals and edge orientation
    (flame.cc:2094-2100); then a third frame in the same manner."""
    pos, data, edges, note = case(name)
    V = len(pos)
    fid = tc.case_ids(V, 0)
    with Frames(env) as fr:
        fr.sync(fid, pos, data, edges)
        fr.check(f"{note}, frame 1")
        next_id = 5 * V + 100
        for frame in (2, 3):
            drop = _must_drop(name, pos, edges) if frame == 2 else []
            new_ids = np.arange(next_id, next_id + V // 8, dtype=np.int32) * 3 + 2
            next_id += V // 8
            fid, pos, data, edges = tc.second_frame(fid, pos, data, edges, drop, new_ids, seed=10 * frame)
            V = len(fid)
            fr.sync(fid, pos, data, edges)
            flat = fr.check_graph(f"{note}, frame {frame}")
            # (not vacuous: some edges survived with their duals, some are new, some survivors run against the caller's orientation)
            assert 0 < int((flat["q1"] != 0).sum()) < flat["E"]
            given = {(int(a), int(b)) for a, b in edges.tolist()}
            assert any((int(d), int(s)) in given for s, d in zip(flat["src"], flat["dst"]))
            fr.run_forms(f"{note}, frame {frame}")


@pytest.mark.gpu
@pytest.mark.parametrize("what", ["hub of 65 edges", "pair listed twice"])
def test_declined_builds_go_the_host_way_and_the_next_frame_is_the_devices_again(env, what):
    """kTopoBadDegree (k_topo_rows: a row of more than 64 half-edges) and kTopoBadEdges (k_topo_new_edges: n_edges != E -- a caller
    that wrongly vouches for edges_unique, the repeated pair joining two SURVIVING vertices, so that the second listing finds the
    previous edge taken by the first): topo_commit declines.  With OPT_SYNC_PATH = 2 that is an error that leaves the previous
    graph, its state and its edge list untouched; with 0 the frame goes the host way (last_sync_path == 1) and equals the
    restatement, which keeps one edge for the pair (flame.cc:2085-2100: boost::edge finds the edge already there).  The declined
    build has moved the device's feature table on: the next, well-formed frame takes the device path again, rebuilds the table
    from the live graph's ids, and finds every survivor."""
    with Frames(env, sync_path=0) as fr:
        if what == "hub of 65 edges":
            pos, data, edges, note = case("hub65")
            fid = tc.case_ids(len(pos), 0)
            bad = (fid, pos, data, edges)
            hub = int(np.argmax(tc.degrees(len(pos), edges)))
        else:
            pos, data, edges, note = case("hubs")
            fid = tc.case_ids(len(pos), 0)
            fr.sync(fid, pos, data, edges)
            fr.check(f"{note}, frame 1")
            f2, p2, d2, e2 = tc.second_frame(fid, pos, data, edges, [], np.arange(9000, 9100, dtype=np.int32), seed=77)
            prev = fr.flat()
            old_pairs = {(min(a, b), max(a, b)) for a, b in zip(fid[prev["src"]].tolist(), fid[prev["dst"]].tolist())}
            k = next(i for i, (a, b) in enumerate(e2.tolist()) if (min(int(f2[a]), int(f2[b])), max(int(f2[a]), int(f2[b]))) in old_pairs)
            e_dup = np.concatenate([e2[:40], e2[k:k + 1, ::-1], e2[40:]]).astype(np.int32)  # the surviving pair once more, the other way round
            bad = (f2, p2, d2, np.ascontiguousarray(e_dup))
            hub = None
        # asked for by name: an error, and nothing has changed
        before, topo_before = fr.flat(), fr.reg.topology()
        fr.sync_path(2)
        with pytest.raises(env.NLTGV2Error):
            fr.reg.sync_graph(bad[0], bad[1], bad[2], np.ones(len(bad[0]), np.float32), bad[3], edges_unique=True)
        assert all(np.array_equal(a, b) for a, b in zip(fr.reg.topology(), topo_before)), f"{what}: the previous edge list"
        assert (fr.reg.info()["V"], fr.reg.info()["E"]) == (before["V"], before["E"])
        assert_state_equal(fr.reg.download_state(), before, keys=ALL_KEYS, what=f"{what}: the previous state after the refused sync")
        # automatic: the host way
        fr.sync_path(0)
        fr.sync(*bad)
        flat = fr.check_graph(f"{what}: declined, host way", path=1)
        if hub is None:
            assert flat["E"] == len(bad[3]) - 1
        else:
            assert fr.reg.info()["max_degree"] == 65
        fr.run_forms(f"{what}: declined, host way", forms=(4, 3))
        # the next frame is well formed (the hub is gone): the device path again
        fid, pos, data, edges = tc.second_frame(bad[0], bad[1], bad[2], flat_edges(flat), [hub] if hub is not None else [],
                                                np.arange(20000, 20080, dtype=np.int32), seed=78)
        fr.sync(fid, pos, data, edges)
        after = fr.check_graph(f"{what}: the frame after", path=2)
        assert int((after["q1"] != 0).sum()) > 0, "survivors were found: their duals came along"
        fr.run_forms(f"{what}: the frame after")


def flat_edges(flat):
    return np.stack([flat["src"], flat["dst"]], 1)


def _delaunay_frame(rng, n):
    pos = np.ascontiguousarray(np.stack([rng.random(n) * 312 + 4, rng.random(n) * 232 + 4], 1), np.float32)
    return pos, (0.5 + rng.random(n)).astype(np.float32)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["host", "device"])
def test_feature_tables_with_colliding_and_returning_ids(env, mode):
    """feat_insert / feat_lookup (nltgv2_topo.hip) with V <= 1024, i.e. two tables of 2^12 slots: 240 ids whose feat_slot is 4093,
    4094 or 4095 (probe chains that wrap from the last slot to slot 0) and 240 that share slot 2048 (one chain of hundreds: the
    compare-and-swap on the stamp hands concurrent inserts consecutive slots, the look-up walks the chain to the first slot of
    another generation).  Four frames of 25 % churn with colliding ids among survivors and newcomers; then six frames in which
    40 ids (colliding ones) are out, in, out, out, in, in: an id that comes back one or two frames later is a NEW vertex
    (flame.cc:2030-2049: not in the graph, so added with VertexData's defaults) although a stale entry of it, two generations
    old, sits in the table it is inserted into.  The host path runs the same sequence for comparison."""
    rng = np.random.default_rng(9)
    coll = tc.colliding_ids(480)
    coll = coll[rng.permutation(480)]
    flicker, pool = coll[:40], list(coll[40:])
    plain = iter(range(50_000, 10_000_000, 37))
    V = 640

    def draw(n, share):
        """n new ids, about `share` of them colliding ones (while the pool lasts)."""
        out = []
        for _ in range(n):
            out.append(int(pool.pop()) if pool and rng.random() < share else next(plain))
        return out

    device = mode == "device"
    flick = flicker.tolist()
    present = [True] * 5 + [False, True, False, False, True, True]  # frame 0 and four frames of churn, then out, in, out, out, in, in
    with Frames(env, sync_path=2 if device else 1) as fr:
        others = draw(V - 40, 0.3)
        for frame, flick_in in enumerate(present):
            newcomers = []
            if frame > 0:
                keep = rng.random(len(others)) > 0.25
                others = [i for i, k in zip(others, keep) if k]
                newcomers = draw(V - 40 - len(others), 0.3)
                others += newcomers
            ids = others + (flick if flick_in else [])
            fid = np.array(ids, np.int32)[rng.permutation(len(ids))]  # the caller's vertex order changes freely
            pos, data = _delaunay_frame(rng, len(fid))
            edges = synth.delaunay_edges_scipy(pos)
            was_in = set(fr.fid.tolist())
            fr.sync(fid, pos, data, edges, edges_unique=device)
            flat = fr.check_graph(f"{mode}, frame {frame}", path=2 if device else 1)
            assert fr.reg.info()["V"] <= 1024
            if 1 <= frame <= 4:
                colliding = set(coll.tolist())
                assert len(colliding & was_in & set(others)) > 20, "colliding ids among the survivors"
                assert len(colliding & set(newcomers)) > 5, "colliding ids among the newcomers"
            if flick_in and not present[frame - 1] and frame > 0:
                # every reappearance is a new vertex, whatever it was when it left one or two frames ago
                assert not set(flick) & was_in
                got = fr.reg.download_state()
                at = np.flatnonzero(np.isin(fid, flicker))
                assert len(at) == 40
                for k in ("x", "x_bar", "x_prev"):
                    assert np.array_equal(got[k][at], data[at]), f"frame {frame}: {k} of a returning id"
                for k in ("w1", "w2", "w1_bar", "w2_bar", "w1_prev", "w2_prev"):
                    assert not got[k][at].any(), f"frame {frame}: {k} of a returning id"
                touching = np.isin(flat["src"], at) | np.isin(flat["dst"], at)
                assert touching.any() and not any(got[q][touching].any() for q in ("q1", "q2", "q3")), f"frame {frame}: duals at a returning id"
            fr.run_forms(f"{mode}, frame {frame}", forms=(4,), runs=(9,))


@pytest.mark.gpu
def test_sync_front_corners_on_the_device_path(env):
    """topo_prepare / k_topo_init / k_topo_edges / the scan / k_topo_new_edges at the ends of their ranges, each by name on the
    device path (OPT_SYNC_PATH = 2):
    Vo = 0 (an empty previous graph: nothing to look up, first_k of one slot);  Eo = 0 with every vertex surviving (old_of_new >= 0
    everywhere, every row of the previous CSR empty);  every previous edge survives and none is new (n_keep == E: the scan's second
    part is all zero, and the result keeps the PREVIOUS order and orientation -- boost::edges() walks a std::list that nothing was
    erased from or appended to, flame.cc:2094-2100);  every vertex survives and no edge does (n_keep == 0 with Eo > 0)."""
    pos, data, edges, _ = case("sized-257")
    V = len(pos)
    fid = tc.case_ids(V, 0)
    none = np.zeros((0, 2), np.int32)
    rng = np.random.default_rng(4)
    with Frames(env, sync_path=0) as fr:
        # -- from an empty graph
        fr.sync(np.zeros(0, np.int32), np.zeros((0, 2), np.float32), np.zeros(0, np.float32), none, edges_unique=False)
        assert (fr.reg.info()["V"], fr.reg.info()["E"]) == (0, 0)
        fr.sync_path(2)
        fr.sync(fid, pos, data, edges)
        fr.check("from an empty graph")
        # -- from an edgeless graph whose vertices all survive
        fr.sync_path(0)
        fr.sync(fid[:50], pos[:50], data[:50], none, edges_unique=False)
        assert (fr.reg.info()["V"], fr.reg.info()["E"]) == (50, 0) and fr.reg.info()["last_sync_path"] == 1
        fr.run_forms("edgeless", forms=(4,), runs=(9,))
        fr.sync_path(2)
        p50 = np.ascontiguousarray(pos[:50] + np.float32(0.25))
        e50 = synth.delaunay_edges_scipy(p50)
        fr.sync(fid[:50], p50, data[:50], e50)
        flat = fr.check_graph("from an edgeless graph")
        assert np.array_equal(flat["x"], fr.reg.download_state()["x"]) and not np.array_equal(flat["x"], data[:50]), "the vertices kept their state"
        fr.run_forms("from an edgeless graph")
        # -- the identical edge list in another order, half of it reversed: all survive, none is new
        fr.sync(fid, pos, data, edges)
        prev = fr.check_graph("back to the full frame")
        fr.run_forms("back to the full frame", forms=(4,), runs=(9,))
        flip = rng.random(len(edges)) < 0.5
        again = np.ascontiguousarray(np.where(flip[:, None], edges[:, ::-1], edges)[rng.permutation(len(edges))])
        fr.sync(fid, pos, data, again)
        flat = fr.check_graph("every edge survives")
        assert np.array_equal(flat["src"], prev["src"]) and np.array_equal(flat["dst"], prev["dst"]), "the previous order and orientation"
        assert np.count_nonzero(flat["q1"]) > flat["E"] // 2
        fr.run_forms("every edge survives")
    # -- the same vertices, a disjoint edge set: no edge survives
    pos, data, edges, _ = case("collinear")
    V = len(pos)
    fid = tc.case_ids(V, 1)
    i = np.arange(V)
    other = np.concatenate([np.stack([i[3:], i[:-3]], 1), np.stack([i[:-4], i[4:]], 1)])
    other = np.ascontiguousarray(other[rng.permutation(len(other))], np.int32)
    with Frames(env, sync_path=2) as fr:
        fr.sync(fid, pos, data, edges)
        fr.check("collinear", forms=(4,))
        before = fr.flat()
        fr.sync(fid, pos, data, other)
        flat = fr.check_graph("no edge survives")
        assert np.array_equal(flat["src"], other[:, 0]) and np.array_equal(flat["dst"], other[:, 1]) and not flat["q1"].any()
        assert np.array_equal(flat["w1"], before["w1"]) and before["w1"].any(), "every vertex kept its state"
        fr.run_forms("no edge survives")


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["forest", "hubs"] + [f"sized-{v}" for v in tc.SIZED_V])
def test_upload_route(env, name):
    """upload_graph's use of the builder (topo_upload: k_topo_edges_given, k_topo_csr_fill, then the same back half) on the same
    shapes, with FLAME_NLTGV2_OPT_PERSISTENT = 4 set before the upload so that the patch-count rule cannot decline: the tables word
    for word the host builders', forms 4 and 3 equal to the checker.
    NOTHING OBSERVABLE PROVES WHICH BUILDER RAN ON THIS ROUTE: upload_graph does not report it, a silent decline to the host
    builders would pass this test, and flame_nltgv2_layout_selftest compares with the host tables either way.  The proof that the
    device builder handles these shapes is the sync route above (last_sync_path == 2 under OPT_SYNC_PATH = 2); this test adds the
    upload front's own kernels in case they ran."""
    from flame_amd.regularizer import OPT_PERSISTENT

    pos, data, edges, note = case(name)
    g = synth.assemble_graph(pos, data, edges)
    ref = synth.copy_graph(g)
    with env.Regularizer(0) as reg:
        reg.set_option(OPT_PERSISTENT, 4)
        reg.upload_graph(g)
        assert reg.layout_selftest() == 0, note
        for form in (4, 3):
            reg.set_option(OPT_PERSISTENT, form)
            for n in RUNS:
                reg.run(env.Params(), n)
                assert oracle.run(ref, n) == 0
                assert_state_equal(reg.download_state(), ref, keys=ALL_KEYS, what=f"{note}: uploaded, form {form}, {n} steps")
