"""FeatureTracker::selectGraphFeatures / getRawIDepths (include/flame_hip/feature_tracker.hpp) and the pointer + count
overloads of DeviceGraph::sync / syncPrepare (include/flame_hip/nltgv2_l1_graph_regularizer.hpp): the program
tests/cpp/select_graph_features_test.cc compiles as C++11 against include/ and, on a GPU, dumps what the facade gave it
for a case written here; the dump is compared bit for bit with the checker (tests/select_ref.py)."""
import os
import struct
import subprocess

import numpy as np
import pytest

from oracle import stereo_capi as so
from tests import frontend_ref as fr
from tests import prune_cases as pc
from tests import select_cases as sc_
from tests import select_ref as sr
from tests.conftest import HAS_GPU, ROOT


def build_program(tmp_path):
    exe = str(tmp_path / "select_graph_features_test")
    lib_dir = os.path.join(ROOT, "flame_amd")
    subprocess.check_call([
        "g++", "-std=c++11", "-O1", "-Wall", "-Wextra", "-Werror", "-Wno-invalid-offsetof", "-I", os.path.join(ROOT, "include"),
        os.path.join(ROOT, "tests", "cpp", "select_graph_features_test.cc"), "-o", exe, "-L", lib_dir, "-lflame_nltgv2_hip",
        f"-Wl,-rpath,{lib_dir}", "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_select_facade_compiles_and_fails_loudly_without_a_device(built, tmp_path):
    exe = build_program(tmp_path)
    if not HAS_GPU:
        r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
        assert r.returncode == 77 and "no usable HIP device" in r.stdout, r.stdout + r.stderr


class Dump:
    def __init__(self, path):
        self.b = open(path, "rb").read()
        self.o = 0

    def take(self, dtype, n):
        a = np.frombuffer(self.b, dtype, n, self.o).copy()
        self.o += a.nbytes
        return a

    def inputs(self):
        V, ex, inv, var, hgt, err = (int(v) for v in self.take("<i4", 6))
        return dict(V=V, num_examined=ex, num_invalid=inv, num_fail_var=var, num_fail_height=hgt, error_feature=err,
                    feat_id=self.take("<i4", V), pos=self.take("<f4", 2 * V).reshape(V, 2), data_term=self.take("<f4", V),
                    data_weight=self.take("<f4", V), feat_index=self.take("<i4", V))


def same(got, ref, what):
    for k in ("V",) + sr.COUNTERS:
        assert got[k] == ref[k], (what, k, got[k], ref[k])
    for k in sr.ARRAYS:
        assert got[k].tobytes() == ref[k].tobytes(), (what, k)


@pytest.mark.gpu
@pytest.mark.parametrize("n, gp, scale", [(8400, dict(), 1.0), (16000, dict(adaptive_data_weights=1, min_height=-0.5, max_height=1.5), 0.37)])
def test_select_facade_dump_equals_the_checker(built, tmp_path, n, gp, scale):
    case = sc_.make(n)
    sc, feats, proj = case["sc"], case["feats"], case["proj"]
    gpf = dict(sr.DEFAULT_GP, **gp)
    # the world is the current camera's frame: pf.pose = the pose relative to frame 23, and fcur.pose the identity
    world = [dict(id=a, q=sc.relative(a, sc_.CUR)[0], t=sc.relative(a, sc_.CUR)[1]) for a in pc.PF_IDS]
    path, dump = str(tmp_path / "case.bin"), str(tmp_path / "dump.bin")
    with open(path, "wb") as f:
        f.write(b"SEL1" + struct.pack("<6i", sc.width, sc.height, n, len(world), sc_.CUR, gpf["adaptive_data_weights"]))
        f.write(np.asarray([gpf["idepth_var_max_graph"], gpf["min_height"], gpf["max_height"], scale], "<f4").tobytes())
        f.write(np.ascontiguousarray(sc.K32, "<f4").tobytes() + np.ascontiguousarray(sc.Kinv32, "<f4").tobytes())
        f.write(np.asarray([p["id"] for p in world], "<u4").tobytes())
        for p in world:
            f.write(np.asarray(p["q"], "<f4").tobytes() + np.asarray(p["t"], "<f4").tobytes())
        f.write(np.ascontiguousarray(feats).tobytes() + np.ascontiguousarray(proj).tobytes())
    r = subprocess.run([build_program(tmp_path), path, dump], capture_output=True, text=True, timeout=300)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and r.stdout.count(": ok") == 3 and "FAIL" not in r.stdout, r.stdout + r.stderr
    d = Dump(dump)
    # 1. the two vectors
    rc, ref = sr.select(feats, proj, sc.Kinv32, world, scale, gp)
    assert rc == 0 and ref["V"] > n // 10
    same(d.inputs(), ref, "vectors")
    # 2. the resident form, against the checker's own projection
    rc, err, kept, cur = fr.project_features(feats, sc_.project_geos(sc), sc_.CUR, sc.width, sc.height)
    assert rc == 0
    rc, ref2 = sr.select(kept, cur, sc.Kinv32, world, scale, gp)
    assert rc == 0 and ref2["V"] > 100
    same(d.inputs(), ref2, "resident")
    # 3. getRawIDepths: the valid records of the projected set (all of them)
    m = int(d.take("<i4", 1)[0])
    assert m == cur.shape[0]
    assert d.take("<f4", 2 * m).tobytes() == np.stack([cur["x"], cur["y"]], 1).astype("<f4").tobytes()
    assert d.take("<f4", m).tobytes() == cur["idepth_mu"].tobytes() and d.take("<f4", m).tobytes() == cur["idepth_var"].tobytes()
    # 4. what the synced graph holds is the selection: its ids, and x = x_bar = the data term of every vertex (a survivor
    # of the seeded half kept it, a new vertex starts there)
    V, E = (int(v) for v in d.take("<i4", 2))
    assert V == ref2["V"] and E >= V
    assert d.take("<i4", V).tobytes() == ref2["feat_id"].tobytes()
    assert d.take("<f4", V).tobytes() == ref2["data_term"].tobytes() and d.take("<f4", V).tobytes() == ref2["data_term"].tobytes()
    assert d.o == len(d.b) and so.FEATURE_DTYPE.itemsize == 40
