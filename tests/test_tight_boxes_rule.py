"""tests/cpp/tight_boxes_tests.cpp: the rule that fits the boxes of the camera- / light-ordered node copies to their live records
(softray_amd/csrc/sr_tight_boxes.h, the text k_tight_level / k_tight_top compile), compiled for the host with AddressSanitizer and
UndefinedBehaviorSanitizer and run on the CPU as a program of its own.  Covered on hand-made four-wide trees: a leaf with no live record,
a subtree with none, a tree with none, nodes with one child, a run that does not lie in its leaf, every depth cut-off from none to all;
on those and on random trees with random runs: every live record's box lies inside every slot above it, a slot is absent exactly when no
live record lies below it, a re-made box is the union of the live boxes below it, and above the cut-off the base boxes stand."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_tight_boxes_rule_on_small_trees(tmp_path):
    exe = str(tmp_path / "tight_boxes_tests")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-o", exe, os.path.join(ROOT, "tests", "cpp", "tight_boxes_tests.cpp")])
    r = subprocess.run([exe, "300"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout
    total = re.search(r"TOTAL slots=(\d+) absent=(\d+) failures=(\d+)", r.stdout)
    assert total, r.stdout
    slots, absent, failures = (int(x) for x in total.groups())
    assert failures == 0
    assert slots > 10000 and absent > 1000                             # present and absent slots were both exercised
