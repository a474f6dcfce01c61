"""The host side of tbc_ledger_realtime (csrc/ledger_rt_plan.h: validation, pairing, statuses, the three streams, the arena) in a
stand-alone program, tests/emu/ledger_rt_plan.cpp, built with -fsanitize=address,undefined and run directly: every shape it plans is
checked against a plain restatement, every refusal message is looked at -- validate's and the plan's own (2^31 micro-ops in one call) --, and the plan is shown never to read a transfer's micro-ops.
The program also holds lgrt::sequence -- the launches the library makes -- over a recording launcher to hand-written lists of (kernel,
grid, threads) on the edge shapes."""
import os
import subprocess

from conftest import ROOT


def test_the_plan_program_under_address_and_undefined_sanitizers(tmp_path):
    exe = str(tmp_path / "ledger_rt_plan")
    subprocess.check_call(["g++", "-std=c++17", "-g", "-O1", "-Wall", "-Wextra", "-Wno-unknown-pragmas", "-Wno-unused-parameter",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "tests", "emu"), "-I", os.path.join(ROOT, "jepsen-tigerbeetle_amd", "csrc"),
                           os.path.join(ROOT, "tests", "emu", "ledger_rt_plan.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "74 ledgers planned and checked, 15 refusals, the launches of 5 shapes" in out.stdout, out.stdout
