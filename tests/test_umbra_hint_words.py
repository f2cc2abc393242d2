"""tests/cpp/umbra_hint_tests.cpp: the hint word of the persistent packet shaft walk (softray_amd/csrc/sr_umbra_hint.h, the text
k_shaft_pkt4 compiles) -- pack, unpack and the bounds rule -- against a scalar model, compiled for the host with AddressSanitizer and
UndefinedBehaviorSanitizer and run on the CPU as a program of its own.  Covered: cn = 0 and 16, cc + cn = nrec and nrec + 1, the absent
word 0xFFFFFFFF for every size of the record array, and random words; every run the rule accepts is read from an array of exactly nrec
records, so an index it lets through stops the program."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_hint_words_against_the_scalar_model(tmp_path):
    exe = str(tmp_path / "umbra_hint_tests")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-o", exe, os.path.join(ROOT, "tests", "cpp", "umbra_hint_tests.cpp")])
    r = subprocess.run([exe, "100000"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout
    total = re.search(r"TOTAL accepted=(\d+) rejected=(\d+) failures=(\d+)", r.stdout)
    assert total, r.stdout
    accepted, rejected, failures = (int(x) for x in total.groups())
    assert failures == 0
    assert accepted > 10000 and rejected > 10000                       # both sides of the rule were exercised
