"""Hunt for histories that take the count form's pipeline (oracle/wgl.py check_count_pipeline) past its budget of 32 probes per op on their
own: the cases of tests/count_form_arms.py were picked from what this prints.  A development tool, not run by the suite.

usage: count_form_arm_hunt.py <first seed> <last seed> [out.jsonl] [--hard]

Every history is columns.pair_events(synth.register_events(**kw)) with 0 .. 2 :ok reads overwritten by a stale-but-plausible value; it is
classified alone (the budget is 32 x its own length) under the wide schedule at widths 2, 4 and 16, under the narrow schedule at 8 and 16
pairs a round, and at width 4 with the relaxed sweep in front.  A line is printed for every arm other than "exact" whose passes stay
under CAP probes in all: the generator's arguments, the overwritten reads, and per schedule the arm, the verdict, the failing op, the
probes summed over the passes and the largest visited set of one pass."""
import json
import os
import random
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from jepsen_tigerbeetle_amd import _native as N, columns, synth      # noqa: E402
from oracle import wgl                                                # noqa: E402

CAS = {"kind": 1, "init": N.NIL}
CAP = 300_000
SCHEDULES = {"w4": (4, 64, False), "w4s": (4, 64, True), "w2": (2, 64, False), "w16": (16, 64, False), "n8": (1, 8, False), "n16": (1, 16, False)}


def history(kw, stale):
    h = columns.pair_events(synth.register_events(**kw))
    for i, v in stale:
        h.a[i] = v
    return h


def ok_reads(h):
    return [i for i in range(len(h)) if h.f[i] == N.F_READ and h.a[i] != N.NIL and h.ret_pos[i] != N.POS_CRASHED]


def classify(d, width, round_pairs, sweep, budget=None, cap=CAP):
    """oracle.check_count_pipeline with every pass after the budgeted one under `cap` probes -> (arm, verdict, failing op, probes summed,
    largest visited set of one pass), or None where the count form does not apply or a pass runs into the cap"""
    seen = [0]
    e = wgl.check_count_pipeline(d, CAS, width=width, budget=budget, round_pairs=round_pairs, relaxed_sweep=sweep, pass_cap=cap,
                                 on_pass=lambda name, r: seen.append(r["visited"]))
    if e is None or e[0] == -1:
        return None
    v, fo, _, tot, arm = e
    if sweep and arm == "exact, no budget":
        arm += " (swept valid)"
    return arm, v, int(fo), tot["probes"], max(seen)


def main():
    args = [a for a in sys.argv[1:] if a != "--hard"]
    hard = "--hard" in sys.argv[1:]
    lo, hi = int(args[0]), int(args[1])
    sink = open(args[2], "a") if len(args) > 2 else sys.stdout
    rng = random.Random(lo)
    t0, seen = time.time(), {}
    for seed in range(lo, hi):
        if hard:          # crowded, crash-heavy, as generated but for stale reads: where the relaxation accepts what the exact counts refuse
            kw = dict(n_ops=rng.choice([40, 60, 100, 200]), n_procs=rng.choice([8, 12, 16, 24]), seed=seed, busy=rng.choice([0.9, 1.0]),
                      info=rng.choice([0.08, 0.15, 0.3, 0.5]), corrupt=0, n_values=rng.choice([2, 3, 5]))
        else:
            kw = dict(n_ops=rng.choice([40, 60, 100, 200, 300, 500, 800]), n_procs=rng.choice([6, 8, 12, 16, 24]), seed=seed, busy=rng.choice([0.3, 0.6, 0.9, 1.0]),
                      info=rng.choice([0.03, 0.08, 0.15, 0.3]), corrupt=rng.choice([0, 0, 0.5, 0.9]), n_values=rng.choice([3, 5]))
        h = history(kw, [])
        rd, r, stale = ok_reads(h), random.Random(seed), []
        for _ in range(rng.choice([1, 1, 2] if hard else [0, 1, 1, 2]) if rd else 0):
            stale.append((r.choice(rd), r.randrange(kw["n_values"])))
        h = history(kw, stale)
        d = h.as_dict()
        arms = {}
        for name, (w, rp, sw) in SCHEDULES.items():
            c = classify(d, w, rp, sw)
            if c is not None and c[0] != "exact":
                arms[name] = c
                seen[c[0]] = seen.get(c[0], 0) + 1
        if arms:
            print(json.dumps({"kw": kw, "stale": stale, "n": len(h), "arms": arms}), file=sink, flush=True)
    print("# seeds", lo, hi, "arms seen", seen, "%.0f s" % (time.time() - t0), file=sys.stderr, flush=True)


if __name__ == "__main__":
    main()
