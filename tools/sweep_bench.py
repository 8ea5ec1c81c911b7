"""armour_sweep measured against the loop it replaces; writes profiles/sweep_bench.json and prints ONE JSON line.

    python tools/sweep_bench.py [--reps 20] [--trials-T 128] [--max-iterations 300] [--no-trials]

* sweep ms (the device time armour_sweep reports: both launches) at S = 64 and 256, for B = 1 (O = 20, T = 100) and B = 128 (O = 50, T = 100),
  medians over --reps calls;
* the yardstick on the same inputs: armour_eval_violations_device with ARMOUR_OPT_CULL_ROWS = 1 enqueued S times on one stream (three launches
  each), timed with events around the S calls -- the existing entry, unchanged;
* the tile size C of the library that ran (armour_sweep_tile()).  Another tile size is another library: sweep.hip compiled with
  -DARMOUR_SWEEP_TILE=c and linked with the other objects, named by the environment variable ARMOUR_HIP_LIB; `--tag c2 --no-trials` then
  writes sweep_bench_c2.json beside the shipped library's file (the committed ones: C = 2, 4, 8);
* solve_rescued on the reference worlds: run_trials with rescue_candidates 0 and 128 -- outcome counts and rescued iterations.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def sweep_against_loop(B, O, T, sizes, reps):
    import torch

    from armour_amd import _lib
    from armour_amd.planner import ArmourNLP, sweep_candidates
    from armour_amd.worlds import random_batch
    bp = random_batch(7000, B, O)
    nlp = ArmourNLP(T=T, limits=_lib.ArmourLimits(max_batch=B, max_obstacles=O)).set_parameters(bp["q0"], bp["qd0"], bp["qdd0"], bp["q_des"], bp["obstacles"])
    nlp.set_option(_lib.OPT_CULL_ROWS, 1)
    listed = nlp.row_relevance()[1]
    dev = torch.device("cuda", 0)
    out = dict(B=B, O=O, T=T, m=int(nlp.m), listed_collision_rows_mean=float(np.mean(listed)), sizes=[])
    for S in sizes:
        cand = sweep_candidates(nlp.n, S)
        for _ in range(3):   # (row lists, buffers, clocks: untimed)
            nlp.sweep(cand)
        sweep_ms = [nlp.sweep(cand)["ms"] for _ in range(reps)]
        ks = torch.tensor(np.repeat(cand[:, None, :], B, axis=1), device=dev)   # [S][B][n]
        rec = torch.zeros((S, B, 32), dtype=torch.uint8, device=dev)
        st = torch.cuda.Stream(device=dev)
        loop_ms = []
        for rep in range(reps + 1):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            for s in range(S):
                nlp.eval_violations_device(ks[s].data_ptr(), rec[s].data_ptr(), st.cuda_stream)
            e1.record(st)
            torch.cuda.synchronize()
            if rep:
                loop_ms.append(e0.elapsed_time(e1))
        sw = nlp.sweep(cand)["records"]
        loop_feasible = rec.cpu().numpy().view(np.int32).reshape(S, B, 8)[:, :, 7].T
        out["sizes"].append(dict(S=S, sweep_ms=float(np.median(sweep_ms)), loop_ms=float(np.median(loop_ms)),
                                 sweep_ms_min_max=[float(np.min(sweep_ms)), float(np.max(sweep_ms))], loop_ms_min_max=[float(np.min(loop_ms)), float(np.max(loop_ms))],
                                 sweep_us_per_candidate=float(np.median(sweep_ms)) * 1e3 / (S * B), loop_us_per_candidate=float(np.median(loop_ms)) * 1e3 / (S * B),
                                 verdicts_agree=bool(np.array_equal(loop_feasible, sw["feasible"])), feasible_fraction=float(sw["feasible"].mean())))
    nlp.close()
    return out


def rescue_trials(T, max_iterations, candidates):
    from armour_amd import scenes
    from armour_amd.trials import OUTCOMES, run_trials
    res = run_trials(scenes.reference_worlds(), T=T, max_iterations=max_iterations, rescue_candidates=candidates)
    s = res["summary"]
    infeasible = sum(1 for w in res["worlds"] for r in w["records"] if not r["feasible"])
    return dict(rescue_candidates=candidates, **{o: s[o] for o in OUTCOMES}, iterations=s["iterations"], rescued_iterations=s["rescued_iterations"],
                infeasible_iterations=infeasible, planning_ms_per_world_iteration=s["planning_ms_per_world_iteration"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--trials-T", type=int, default=128)
    ap.add_argument("--max-iterations", type=int, default=300)
    ap.add_argument("--no-trials", action="store_true")
    ap.add_argument("--tag", default="")
    a = ap.parse_args()
    from armour_amd import _lib
    out = dict(tile=int(_lib.load().armour_sweep_tile()), shapes=[sweep_against_loop(1, 20, 100, (64, 256), a.reps), sweep_against_loop(128, 50, 100, (64, 256), a.reps)])
    if not a.no_trials:
        out["trials"] = [rescue_trials(a.trials_T, a.max_iterations, c) for c in (0, 128)]
    path = os.path.join(ROOT, "profiles", f"sweep_bench{('_' + a.tag) if a.tag else ''}.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
