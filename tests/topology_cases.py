"""Graphs that are NOT one Delaunay frame, for the device topology builder (flame_amd/csrc/nltgv2_topo.hip): tests/test_topology_builder_edges.py
feeds them to it.  numpy (and scipy's Delaunay for `sized`) only, no GPU, every generator deterministic for its seed.

Every generator returns (pos (V,2) f32, data_term (V,) f32, edges (E,2) i32, note).  The edge list is shuffled and its orientation is
mixed, so a row's ascending-edge-id order (k_topo_rows) is not its insertion order; every edge joins two vertices at DIFFERENT
positions (the sync sets alpha = 1 / length); no pair is listed twice."""
from __future__ import annotations

import numpy as np

from flame_amd import synth

F = np.float32
WIDTH, HEIGHT = 320.0, 240.0
HUB_DEGREES = (8, 9, 16, 17, 32, 33, 48, 49, 63, 64)   # the thresholds of walk_place, one hub each
SIZED_V = (2, 3, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025)  # slice / kWalkSegment / kWindow at n-1, n, n+1; cc_bits 1 and 2


def _finish(pos, data, edges, rng, note, reverse=None):
    """Mixed orientation (`reverse`: a mask, default a fair coin per edge), shuffled order."""
    e = np.asarray(edges, np.int64).reshape(-1, 2)
    flip = (rng.random(len(e)) < 0.5) if reverse is None else np.asarray(reverse, bool)
    e = np.where(flip[:, None], e[:, ::-1], e)
    e = e[rng.permutation(len(e))]
    return np.ascontiguousarray(pos, F), np.ascontiguousarray(data, F), np.ascontiguousarray(e, np.int32), note


def _data(rng, n):
    return (0.5 + rng.random(n)).astype(F)


def degrees(V, edges):
    return np.bincount(np.asarray(edges).reshape(-1), minlength=V)[:V] if len(edges) else np.zeros(V, np.int64)


def components(V, edges):
    """Label of every vertex = the smallest vertex id of its connected component (what the host's union-find and k_topo_roots give)."""
    parent = np.arange(V)

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a

    for a, b in np.asarray(edges).reshape(-1, 2).tolist():
        ra, rb = find(a), find(b)
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)
    return np.array([find(v) for v in range(V)])


def case_ids(V, seed):
    """Feature ids of a case: scattered, not growing with the vertex index, none of them 3 or 4 (the seed graph's, SEED_IDS)."""
    return (np.random.default_rng(1000 + seed).permutation(V) * 5 + 11).astype(np.int32)


SEED_IDS = np.array([3, 4], np.int32)


def seed_graph():
    """The two-vertex graph a context holds before a case is synced in: none of its ids is a case's, so every vertex of the case is
    new and the builder builds the whole topology."""
    return synth.assemble_graph(np.array([[1.0, 1.0], [5.0, 4.0]], F), np.array([0.75, 1.25], F), np.array([[1, 0]], np.int32))


# ---- the families ------------------------------------------------------------------------------------------------------------------
def path(V, seed=1):
    """One path laid along a jittered snake, every third edge reversed: the longest chain a graph of V vertices has -- the worst case
    for the smallest-neighbour round of k_topo_rows and for the hooking rounds (k_topo_hook_min, k_topo_hook)."""
    rng = np.random.default_rng(seed)
    W = int(np.ceil(np.sqrt(V * WIDTH / HEIGHT)))
    i = np.arange(V)
    r, c = i // W, i % W
    c = np.where(r % 2 == 1, W - 1 - c, c)
    step = min((WIDTH - 8) / W, (HEIGHT - 8) / (V // W + 1))
    pos = np.stack([c, r], 1) * step + 2 + rng.random((V, 2)) * 0.4 * step
    e = np.stack([i[:-1], i[1:]], 1)
    return _finish(pos, _data(rng, V), e, rng, f"path of {V}", reverse=np.arange(V - 1) % 3 == 2)


_SMALL = {1: [], 2: [(0, 1)], 3: [(0, 1), (1, 2), (2, 0)], 5: [(0, 1), (0, 2), (2, 3), (3, 4)]}  # size -> edges (3: a triangle; 5: a tree)


def forest(n_components=700, with_grid=False, seed=2):
    """A disjoint union of components of 1, 1, 2, 2, 3 (a triangle) and 5 vertices, repeated; positions scrambled over the image, so
    components interleave in Morton order while the walk keeps each together.

    The walk orders components by their label, the smallest vertex id (k_topo_roots, WalkKey).  Every component's smallest id is
    handed out first, the singles and pairs before the others: ids 0 .. n_components-1 are one vertex of each component, in the
    order single, pair, single, pair, ...; then triangle, five, ...  So the first 512-window of the walk holds ~340 component
    borders (more than 255: the `run << 16` field of k_topo_windows), isolated vertices stand between connected ones, and every
    component is smaller than a patch.  The other vertices get the remaining ids at random.

    with_grid: a 30 x 20 four-neighbour grid component whose smallest id lies after the first 100 components -- it starts around
    walk position 150 and covers positions 256 and 512: a segment of k_topo_walk and a window of k_topo_windows BEGIN inside it."""
    rng = np.random.default_rng(seed)
    sizes = [(1, 1, 2, 2, 3, 5)[k % 6] for k in range(n_components)]
    singles, pairs = ([k for k, s in enumerate(sizes) if s == n] for n in (1, 2))
    order = [k for sp in zip(singles, pairs) for k in sp] + [k for k, s in enumerate(sizes) if s > 2]  # by label: single, pair, single, pair, ...
    grid_at = 100 if with_grid else -1
    GW, GH = 30, 20
    n_small = sum(sizes)
    V = n_small + (GW * GH if with_grid else 0)
    # labels: one vertex of each component, in walk order
    first_id = {}
    nxt = 0
    for rank, k in enumerate(order):
        if rank == grid_at:
            grid_first = nxt
            nxt += 1
        first_id[k] = nxt
        nxt += 1
    rest = list(rng.permutation(np.arange(nxt, V)))
    edges = []
    for k, s in enumerate(sizes):
        ids = [first_id[k]] + [int(rest.pop()) for _ in range(s - 1)]
        edges += [(ids[a], ids[b]) for a, b in _SMALL[s]]
    pos = np.stack([rng.random(V) * (WIDTH - 8) + 4, rng.random(V) * (HEIGHT - 8) + 4], 1)
    if with_grid:
        gid = np.array([grid_first] + [int(v) for v in rest])
        rng.shuffle(gid[1:])
        assert len(gid) == GW * GH
        gi, gj = np.meshgrid(np.arange(GW), np.arange(GH))
        pos[gid] = np.stack([gi.ravel(), gj.ravel()], 1) * 7.0 + 40 + rng.random((GW * GH, 2)) * 3.0
        at = lambda x, y: int(gid[y * GW + x])  # noqa: E731
        for y in range(GH):
            for x in range(GW):
                if x + 1 < GW:
                    edges.append((at(x, y), at(x + 1, y)))
                if y + 1 < GH:
                    edges.append((at(x, y), at(x, y + 1)))
    note = f"forest of {n_components} components" + (" around a 30x20 grid" if with_grid else "")
    return _finish(pos, _data(rng, V), edges, rng, note)


def grid_with_hubs(hub_degrees=HUB_DEGREES, seed=3):
    """A jittered 40 x 30 four-neighbour grid with one hub per requested degree; spokes go to vertices that stay below 8 edges (as
    grid_with_one_hub of tests/test_pv_lean.py), so every hub has exactly its degree and nobody else reaches 8."""
    rng = np.random.default_rng(seed)
    W, H = 40, 30
    V = W * H
    ii, jj = np.meshgrid(np.arange(W), np.arange(H))
    pos = np.stack([ii.ravel(), jj.ravel()], 1) * 7.5 + 4 + rng.random((V, 2)) * 3.0
    vid = lambda x, y: y * W + x  # noqa: E731
    edges = []
    for y in range(H):
        for x in range(W):
            if x + 1 < W:
                edges.append((vid(x, y), vid(x + 1, y)))
            if y + 1 < H:
                edges.append((vid(x, y), vid(x, y + 1)))
    deg = degrees(V, edges)
    # hubs: interior vertices spread over the grid, no two adjacent
    hubs = [vid(3 + 7 * (k % 5) + (k // 5), 5 + 9 * (k // 5) + 2 * (k % 5)) for k in range(len(hub_degrees))]
    assert len(set(hubs)) == len(hubs) and all(deg[h] == 4 for h in hubs)
    pairs = {(min(a, b), max(a, b)) for a, b in edges}
    for h, want in zip(hubs, hub_degrees):
        for v in rng.permutation(V).tolist():
            if deg[h] >= want:
                break
            if v == h or v in hubs or deg[v] >= 7 or (min(h, v), max(h, v)) in pairs:
                continue
            edges.append((h, v))
            pairs.add((min(h, v), max(h, v)))
            deg[h] += 1
            deg[v] += 1
        assert deg[h] == want
    return _finish(pos, _data(rng, V), edges, rng, f"40x30 grid with hubs of {tuple(hub_degrees)}")


_FULL = {}


def sized(V, seed=4):
    """A jittered-grid Delaunay triangulation cut to exactly its first V vertices (row-major), with its edges restricted to them."""
    if seed not in _FULL:
        p = synth.make_points(320, 240, 6, seed)
        _FULL[seed] = (p, synth.delaunay_edges_scipy(p))
    p, e = _FULL[seed]
    assert V <= len(p)
    rng = np.random.default_rng(seed * 7919 + V)
    e = e[(e[:, 0] < V) & (e[:, 1] < V)]
    return _finish(p[:V], _data(rng, V), e, rng, f"Delaunay cut to {V}")


def collinear(V, seed=5):
    """All vertices on one horizontal line (sy == 0 in topo_prepare: the Morton code of k_topo_init comes from x alone), x strictly
    increasing; path edges plus the chords i -> i + 2."""
    rng = np.random.default_rng(seed)
    x = np.cumsum(0.5 + rng.random(V)) * (WIDTH - 8) / (1.5 * V) + 4
    assert np.all(np.diff(x.astype(F)) > 0)
    pos = np.stack([x, np.full(V, 117.25)], 1)
    i = np.arange(V)
    e = np.concatenate([np.stack([i[:-1], i[1:]], 1), np.stack([i[:-2], i[2:]], 1)])
    return _finish(pos, _data(rng, V), e, rng, f"{V} collinear vertices")


def stacked(W=30, H=20, seed=6):
    """A jittered four-neighbour grid in which a quarter of the vertices lie exactly on a NON-ADJACENT vertex: equal Morton codes
    inside one component, so the stability of the radix sort (ascending vertex id) decides the walk."""
    rng = np.random.default_rng(seed)
    V = W * H
    ii, jj = np.meshgrid(np.arange(W), np.arange(H))
    pos = np.stack([ii.ravel(), jj.ravel()], 1) * 9.0 + 6 + rng.random((V, 2)) * 4.0
    edges = []
    for y in range(H):
        for x in range(W):
            if x + 1 < W:
                edges.append((y * W + x, y * W + x + 1))
            if y + 1 < H:
                edges.append((y * W + x, (y + 1) * W + x))
    adj = {(min(a, b), max(a, b)) for a, b in edges}
    cand = rng.permutation(V).tolist()
    moved = 0
    while moved < V // 4:
        u, v = cand.pop(), cand.pop()  # v moves onto u; each vertex takes part in one pair at most
        if (min(u, v), max(u, v)) in adj:
            cand.insert(0, u), cand.insert(0, v)
            continue
        pos[v] = pos[u]
        moved += 1
    return _finish(pos, _data(rng, V), edges, rng, f"{W}x{H} grid, {moved} vertices stacked on another")


def feat_slot(ids, bits):
    """== feat_slot of flame_amd/csrc/nltgv2_topo.hip, restated: ((uint32)id * 0x9E3779B1u) >> (32 - bits)."""
    return ((np.asarray(ids, np.uint64) * np.uint64(0x9E3779B1)) & np.uint64(0xFFFFFFFF)) >> np.uint64(32 - bits)


def colliding_ids(n, bits=12):
    """n feature ids below 2^31, found by brute force over 0, 1, 2, ...: the first half hash (feat_slot above, the restatement of
    nltgv2_topo.hip's) into the LAST THREE slots of a table of 2^bits slots -- their probe chains wrap from the last slot to
    slot 0 --, the second half all into ONE slot in the middle, 2^(bits-1) -- one probe chain of n / 2 entries.
    A fresh context whose graphs have V, Vo <= 1024 has tables of 2^12 slots (topo_prepare: `int bits = 12; while ((1 << bits) <
    4 * max(V, Vo)) ++bits`, and the tables never shrink), which is the default here."""
    n_tail, n_mid = n - n // 2, n // 2
    tail, mid = [], []
    lo, chunk = 0, 1 << 21
    while (len(tail) < n_tail or len(mid) < n_mid) and lo < (1 << 31) - chunk:
        ids = np.arange(lo, lo + chunk, dtype=np.uint64)
        s = feat_slot(ids, bits)
        tail += ids[s >= np.uint64((1 << bits) - 3)].tolist()
        mid += ids[s == np.uint64(1 << (bits - 1))].tolist()
        lo += chunk
    assert len(tail) >= n_tail and len(mid) >= n_mid
    return np.array(tail[:n_tail] + mid[:n_mid], np.int32)


# ---- a second frame on a graph that is not a triangulation ---------------------------------------------------------------------------
def second_frame(fid, pos, data, edges, must_drop, new_ids, seed, drop=0.15, max_degree_of_new_neighbours=6):
    """The frame after (fid, pos, data, edges): drops ~`drop` of the vertices (all of `must_drop` among them: whole small components,
    a hub), moves the survivors a little (projectGraph), permutes the caller's vertex order, reverses half of the edges, leaves
    out a tenth of the surviving pairs, joins some surviving vertices by pairs that were no edge, and adds len(new_ids) new vertices,
    each tied to one or two vertices of small degree.  -> (fid, pos, data, edges) of the new frame; no pair twice, no edge of length 0."""
    rng = np.random.default_rng(seed)
    V = len(fid)
    keep = rng.random(V) > drop
    keep[np.asarray(must_drop, np.int64)] = False
    n_keep, n_new = int(keep.sum()), len(new_ids)
    new_index = np.full(V, -1)
    new_index[keep] = np.arange(n_keep)
    p = np.concatenate([pos[keep] + rng.normal(0, 0.2, (n_keep, 2)), np.stack([rng.random(n_new) * (WIDTH - 8) + 4, rng.random(n_new) * (HEIGHT - 8) + 4], 1)])
    d = np.concatenate([data[keep] + rng.normal(0, 0.01, n_keep), _data(rng, n_new)])
    f = np.concatenate([fid[keep], np.asarray(new_ids, np.int32)])
    e = new_index[np.asarray(edges, np.int64)]
    e = e[(e[:, 0] >= 0) & (e[:, 1] >= 0)]
    e = e[rng.random(len(e)) > 0.1]
    pairs = {(min(a, b), max(a, b)) for a, b in e.tolist()}
    deg = degrees(n_keep + n_new, e)
    extra = []

    def join(a, b):
        if a != b and (min(a, b), max(a, b)) not in pairs and deg[a] <= max_degree_of_new_neighbours and deg[b] <= max_degree_of_new_neighbours:
            pairs.add((min(a, b), max(a, b)))
            extra.append((a, b))
            deg[a] += 1
            deg[b] += 1

    for _ in range(n_keep // 10):
        join(int(rng.integers(n_keep)), int(rng.integers(n_keep)))
    for v in range(n_keep, n_keep + n_new):
        for _ in range(int(rng.integers(1, 3))):
            join(v, int(rng.integers(n_keep + n_new)))
    e = np.concatenate([e, np.array(extra, np.int64).reshape(-1, 2)])
    order = rng.permutation(n_keep + n_new)       # the caller's vertex order changes freely
    where = np.empty_like(order)
    where[order] = np.arange(len(order))
    p, d, e, _ = _finish(p[order], d[order], where[e], rng, "")
    return np.ascontiguousarray(f[order], np.int32), p, d, e
