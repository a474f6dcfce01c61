"""The host side of tbc_ledger_journal (csrc/ledger_journal_plan.h: validation, the three groups of gathered columns, the owner columns,
the slices, the arena) in a stand-alone program, tests/emu/ledger_journal_plan.cpp, built with -fsanitize=address,undefined and run
directly: every shape it plans is checked against a plain restatement, the plan's own refusals are looked at -- 2^31 transfer micro-ops,
2^31 entries a lookup, lookups x words of 2^31, reads x counters of 2^31 --, and the plan is shown never to read a micro-op.  The program
includes the emulator build of the kernels, so each planned ledger also runs through every kernel under the sanitizers, into output
arrays of exactly the stated sizes; and it holds the launch sequence the library runs over a recording launcher to hand-written lists of
(kernel, grid, threads): launch for launch, and no launch for an empty phase."""
import os
import subprocess

from conftest import ROOT


def test_the_plan_program_under_address_and_undefined_sanitizers(tmp_path):
    exe = str(tmp_path / "ledger_journal_plan")
    subprocess.check_call(["g++", "-std=c++17", "-g", "-O1", "-Wall", "-Wextra", "-Wno-unknown-pragmas", "-Wno-unused-parameter",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "tests", "emu"), "-I", os.path.join(ROOT, "jepsen-tigerbeetle_amd", "csrc"),
                           os.path.join(ROOT, "tests", "emu", "ledger_journal_plan.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "49 ledgers planned, run and checked, 8 refusals, the launches of 7 shapes" in out.stdout, out.stdout
