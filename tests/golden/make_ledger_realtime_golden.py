"""Writes tests/golden/ledger_realtime/<name>.edn + <name>.json: one small history per rule and boundary of the realtime bounds
(jepsen/ledger.py), with every array the checker gives.  THE EXPECTED ARRAYS BELOW ARE WRITTEN BY HAND -- README.md in that directory
derives each -- and nothing here calls the checker: tests/test_ledger_realtime_host.py compares the host statement with these files.
Run from the repository root:  python tests/golden/make_ledger_realtime_golden.py"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from jepsen_tigerbeetle_amd.jepsen import edn  # noqa: E402

MIN, MAX = -(2 ** 63), 2 ** 63 - 1
NONE = [MIN, MIN]
X = [["t", 1, {"debit-acct": 1, "credit-acct": 2, "amount": 5}]]           # the transfer most fixtures use: 5 from account 1 to account 2


def op(p, typ, value):
    return {"type": typ, "f": "txn", "value": value, "process": p}


def rinv(p, ids=(1, 2)):
    return op(p, "invoke", [["r", a, None] for a in ids])


def rok(p, *mops):
    return op(p, "ok", [["r", a, None if m is None else {"credits-posted": m[0], "debits-posted": m[1]}] for a, m in mops])


ZERO = ((1, (0, 0)), (2, (0, 0)))
AFTER_X = ((1, (0, 5)), (2, (5, 0)))
FIXTURES = {
    # name: (history, opts, bits per read, miss per read, lo, hi, floor per read micro-op, summary counts)
    "transfer-returns-just-before-read-invoked": (
        [op(0, "invoke", X), op(0, "ok", X), rinv(1), rok(1, *ZERO)], {},
        [3], [[5, 0, 0]], [[0, 5], [5, 0]], [[0, 5], [5, 0]], [NONE, NONE], {"n_definite": 1, "n_possible": 1}),
    "transfer-returns-just-after-read-invoked": (
        [op(0, "invoke", X), rinv(1), op(0, "ok", X), rok(1, *ZERO)], {},
        [0], [[0, 0, 0]], [[0, 0], [0, 0]], [[0, 5], [5, 0]], [NONE, NONE], {"n_definite": 1}),
    "transfer-invoked-just-before-read-returns": (
        [rinv(1), op(0, "invoke", X), rok(1, *AFTER_X), op(0, "ok", X)], {},
        [0], [[0, 0, 0]], [[0, 0], [0, 0]], [[0, 5], [5, 0]], [NONE, NONE], {}),
    "transfer-invoked-just-after-read-returns": (
        [rinv(1), rok(1, *AFTER_X), op(0, "invoke", X), op(0, "ok", X)], {},
        [12], [[0, 5, 0]], [[0, 0], [0, 0]], [[0, 0], [0, 0]], [NONE, NONE], {}),
    "read-without-invocation": (
        [op(0, "invoke", X), op(0, "ok", X), rinv(2, (1,)), rok(2, (1, (0, 5))), rok(1, *ZERO)], {},
        [0, 0], [[0, 0, 0], [0, 0, 0]], [[0, 5], [0, 0], [0, 0]], [[0, 5], [0, 5], [5, 0]], [NONE, NONE, NONE], {"read_count": 2}),
    "open-transfer": (
        [op(0, "invoke", X), rinv(1), rok(1, *AFTER_X), rinv(1), rok(1, *ZERO)], {},
        [0, 48], [[0, 0, 0], [0, 0, 5]], [[0, 0]] * 4, [[0, 5], [5, 0], [0, 5], [5, 0]], [NONE, NONE, [0, 5], [5, 0]], {"n_definite": 0, "n_possible": 1}),
    "failed-transfer": (
        [op(0, "invoke", X), op(0, "fail", X), rinv(1), rok(1, *AFTER_X)], {},
        [12], [[0, 5, 0]], [[0, 0], [0, 0]], [[0, 0], [0, 0]], [NONE, NONE], {"n_definite": 0, "n_possible": 0}),
    "self-transfer": (
        [op(0, "invoke", [["t", 1, {"debit-acct": 1, "credit-acct": 1, "amount": 4}]]), op(0, "ok", [["t", 1, {"debit-acct": 1, "credit-acct": 1, "amount": 4}]]),
         rinv(1, (1,)), rok(1, (1, (4, 4)))], {},
        [0], [[0, 0, 0]], [[4, 4]], [[4, 4]], [NONE], {}),
    "amount-zero": (
        [op(0, "invoke", [["t", 1, {"debit-acct": 1, "credit-acct": 2, "amount": 0}]]), op(0, "ok", [["t", 1, {"debit-acct": 1, "credit-acct": 2, "amount": 0}]]),
         rinv(1), rok(1, *ZERO)], {},
        [0], [[0, 0, 0]], [[0, 0], [0, 0]], [[0, 0], [0, 0]], [NONE, NONE], {"n_definite": 1}),
    "foreign-account-on-one-side": (
        [op(0, "invoke", [["t", 1, {"debit-acct": 1, "credit-acct": 99, "amount": 5}]]), op(0, "ok", [["t", 1, {"debit-acct": 1, "credit-acct": 99, "amount": 5}]]),
         rinv(1), rok(1, (1, (0, 5)), (2, (0, 0)))], {},
        [0], [[0, 0, 0]], [[0, 5], [0, 0]], [[0, 5], [0, 0]], [NONE, NONE], {"foreign_sides": 1}),
    "nil-and-unknown-micro-ops": (
        [op(0, "invoke", X), op(0, "ok", X), rinv(1, (1, 77, 2)), rok(1, (1, None), (77, (9, 9)), (2, (5, 0)))], {},
        [0], [[0, 0, 0]], [NONE, NONE, [5, 0]], [NONE, NONE, [5, 0]], [NONE, NONE, NONE], {"n_checked": 1}),
    "repeated-id-within-a-read": (
        [op(0, "invoke", X), op(0, "ok", X), rinv(1, (2, 1, 2)), rok(1, (2, (0, 0)), (1, (0, 5)), (2, (5, 0)))], {},
        [0], [[0, 0, 0]], [[5, 0], [0, 5]], [[5, 0], [0, 5]], [NONE, NONE], {"n_checked": 2}),
    "ok-transfers-apply-false": (
        [op(0, "invoke", X), op(0, "ok", X), rinv(1), rok(1, *ZERO)], {"ok-transfers-apply?": False},
        [0], [[0, 0, 0]], [[0, 0], [0, 0]], [[0, 5], [5, 0]], [NONE, NONE], {}),
    "nonzero-initial": (
        [op(0, "invoke", X), op(0, "ok", X), rinv(1), rok(1, (1, (100, 10)), (2, (50, 0)))],
        {"initial": {1: {"credits-posted": 100, "debits-posted": 10}, 2: {"credits-posted": 50, "debits-posted": 0}}},
        [3], [[5, 0, 0]], [[100, 15], [55, 0]], [[100, 15], [55, 0]], [NONE, NONE], {}),
    "value-at-int64-min": (
        [op(0, "invoke", X), op(0, "ok", X), rinv(1, (2,)), rok(1, (2, (MIN, 0)))], {},
        [1], [[MAX, 0, 0]], [[5, 0]], [[5, 0]], [NONE], {}),
}


def main():
    out = os.path.join(HERE, "ledger_realtime")
    for name, (history, opts, bits, miss, lo, hi, floor, counts) in FIXTURES.items():
        history = [dict(o, index=i, time=1000000 * i) for i, o in enumerate(history)]
        edn.write_history(os.path.join(out, name + ".edn"), history)
        o = {"accounts": [1, 2], **{k: v for k, v in opts.items() if k != "initial"}}
        if "initial" in opts:
            o["initial"] = [[a, m["credits-posted"], m["debits-posted"]] for a, m in opts["initial"].items()]      # (JSON has no integer keys)
        with open(os.path.join(out, name + ".json"), "w") as f:
            json.dump({"opts": o, "bits": bits, "miss": miss, "lo": lo, "hi": hi, "floor": floor, "counts": counts}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
