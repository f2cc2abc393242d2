"""tests/cpp/light_cone_tests.cpp: the penumbra-plane filter of the packet shaft walk (softray_amd/csrc/sr_light_cone.h, the text that
k_light_cones and k_shaft_pkt4 compile) against FP64 ground truth, compiled for the host and run on the CPU.  The program exits 0 only if
the filter never rejects a (triangle, surface point) pair for which some sample ray of the light ball hits, never says umbra for a pair
where some sample misses, and every verdict and both ground-truth classes occurred."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_filter_is_conservative_against_fp64_ground_truth(tmp_path):
    exe = str(tmp_path / "light_cone_tests")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-ffp-contract=off", "-o", exe, os.path.join(ROOT, "tests", "cpp", "light_cone_tests.cpp")])
    r = subprocess.run([exe, "600"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout
    total = re.search(r"TOTAL pairs=(\d+) some_hit=(\d+) all_hit=(\d+) rejected=(\d+) umbra=(\d+) .* violations=(\d+)", r.stdout)
    assert total, r.stdout
    pairs, some_hit, all_hit, rejected, umbra, violations = (int(x) for x in total.groups())
    assert violations == 0
    assert pairs == 8 * 600 * 4 and some_hit > pairs // 10 and all_hit > pairs // 50 and rejected > pairs // 4 and umbra > pairs // 50
    # every special class ran, and the always-pass classes really keep pairs the TriSlab filter rejects
    for name in ("ball straddles the plane", "ball touches an edge line", "R = 0", "light 1e3 x extent away", "points 1e-6 from the plane",
                 "points near an edge line"):
        assert name in r.stdout
