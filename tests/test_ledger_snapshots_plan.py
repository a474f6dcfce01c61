"""The host side of tbc_ledger_snapshots (csrc/ledger_snap_plan.h: validation, the reads' rows, the gathered columns, the chunks, the
arena) in a stand-alone program, tests/emu/ledger_snap_plan.cpp, built with -fsanitize=address,undefined and run directly: every shape
it plans is checked against a plain restatement, every refusal message is looked at -- validate's and the plan's own two (reads x
counters of 2^31, 2^31 micro-ops of reads) --, and the plan is shown never to read a micro-op.  The program includes the emulator build
of the kernels, so each planned ledger also runs through every kernel under the sanitizers and is held to the rules restated pair by
pair; and it holds the two launch sequences the library runs over a recording launcher to hand-written lists of (kernel, grid,
threads) on the edge shapes."""
import os
import subprocess

from conftest import ROOT


def test_the_plan_program_under_address_and_undefined_sanitizers(tmp_path):
    exe = str(tmp_path / "ledger_snap_plan")
    subprocess.check_call(["g++", "-std=c++17", "-g", "-O1", "-Wall", "-Wextra", "-Wno-unknown-pragmas", "-Wno-unused-parameter",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "tests", "emu"), "-I", os.path.join(ROOT, "jepsen-tigerbeetle_amd", "csrc"),
                           os.path.join(ROOT, "tests", "emu", "ledger_snap_plan.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "50 ledgers planned, run and checked, 11 refusals, the launches of 4 shapes" in out.stdout, out.stdout
