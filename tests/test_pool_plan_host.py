"""What a pass zeroes of a batch's growth pool (csrc/pool_plan.h: all of it where the memory is new or the visited sets start over, else
the words the searches were handed) in its stand-alone program, tests/emu/pool_plan.cpp, built with -fsanitize=address,undefined: a
model of the device's pool and cursor through the events of a batch's life, every word zero before every search."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_pool_plan_program_under_address_and_undefined_sanitizers(tmp_path):
    exe = str(tmp_path / "pool_plan")
    subprocess.check_call(["g++", "-std=c++17", "-g", "-O1", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", os.path.join(ROOT, "jepsen-tigerbeetle_amd", "csrc"), os.path.join(ROOT, "tests", "emu", "pool_plan.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "passes checked" in out.stdout and not out.stderr, (out.stdout, out.stderr)
