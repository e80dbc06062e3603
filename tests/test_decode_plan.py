"""The decode routes as a value (trpx_amd/csrc/decode_plan.hpp): CPU tier, no library loaded."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_routes_named_by_the_plan():
    """Every entry point's route for the stacks of DESIGN.md 4.6, under ASan + UBSan (a stand-alone CPU program)."""
    cpp = os.path.join(ROOT, "tests", "cpp")
    subprocess.check_call(["make", "-s", "-C", cpp, "-f", "decode_plan_test.mk"])   # (make: rebuilt when the header changed)
    r = subprocess.run([os.path.join(cpp, "decode_plan_test")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "OK decode plan" in r.stdout, r.stdout + r.stderr
