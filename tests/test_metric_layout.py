"""MetricLayout (flame_amd/csrc/side_stage.hpp): tests/cpp/metric_layout_test.cc is a stand-alone program that walks every
combination of the want_* flags -- offsets 16-byte aligned, no overlap, `total` covers everything -- compiled with AddressSanitizer
and UndefinedBehaviorSanitizer and run directly.  Nothing is loaded into Python."""
import os
import subprocess

from tests.conftest import ROOT


def test_metric_layout_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "metric_layout_test")
    subprocess.check_call(["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra",
                           "-Werror", "-I", os.path.join(ROOT, "flame_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "metric_layout_test.cc"),
                           "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "384 layouts walked, 0 violations" in r.stdout, r.stdout + r.stderr
