"""The host side of tbc_ledger_cycles (csrc/ledger_cycles_plan.h: validation, the snapshot plan, inv and ret by pairing, the arena) and
its kernels in a stand-alone program, tests/emu/ledger_cycles_plan.cpp, built with -fsanitize=address,undefined and run directly:
every ledger it plans runs through every kernel under the sanitizers and is held to a plain restatement of the rules (the explicit
graph and its transitive closure); the refusal messages are looked at; the launches of a history without a core are held to a
hand-written list."""
import os
import subprocess

from conftest import ROOT


def test_the_plan_program_under_address_and_undefined_sanitizers(tmp_path):
    exe = str(tmp_path / "ledger_cycles_plan")
    subprocess.check_call(["g++", "-std=c++17", "-g", "-O1", "-Wall", "-Wextra", "-Wno-unknown-pragmas", "-Wno-unused-parameter",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "tests", "emu"), "-I", os.path.join(ROOT, "jepsen-tigerbeetle_amd", "csrc"),
                           os.path.join(ROOT, "tests", "emu", "ledger_cycles_plan.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "60 ledgers planned, run and checked, 3 refusals, the launches of 1 shape" in out.stdout, out.stdout
