"""Throughput of bf_rts_smoother_f32 at the headline shape (n = 4, m = 2, B = 65 536, T = 10 000, reference layout).

Inputs are the streams the headline Kalman filter writes.  Each mode is warmed up, then timed with device events over
at least one second of work.  Algorithmic bytes per trajectory-step: full streams 160 read + 80 written, recompute
(filtered streams only) 80 + 80, plus 64 written with cross-covariances.  Also the filter + smoother pair end to end.
One JSON line per measurement.  Usage: python scripts/smoother_probe.py [--B 65536] [--T 10000] [--min-seconds 1]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bayesianfiltering_amd as bfa  # noqa: E402
from tests import common as cm  # noqa: E402

SPEC_BPS = 8.0e12


def timed(fn, min_seconds, warmup=2):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    once = e0.elapsed_time(e1) / 1e3
    reps = max(1, int(np.ceil(min_seconds / max(once, 1e-6))))
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / 1e3 / reps, reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=65536)
    ap.add_argument("--T", type=int, default=10000)
    ap.add_argument("--min-seconds", type=float, default=1.0)
    ap.add_argument("--modes", default="full,strided,recompute,full_cross")
    args = ap.parse_args()
    B, T, n = args.B, args.T, 4
    a = cm.cv_model_arrays()
    p = cm.product_params(a)
    y = torch.randn((B, T, 2), device="cuda") * 0.3
    init = np.tile(a["m0"], (B, 1))
    post = bfa.kalman_filter(p, y, initial_means=init, fields=("means", "covariances", "predicted_means", "predicted_covariances"))
    filt_only = post._replace(predicted_means=None, predicted_covariances=None)
    out = bfa.rts_smoother(p, post)
    out_c = None
    steps = B * T
    cases = {
        "full": (lambda: bfa.rts_smoother(p, post, out=out), 160 + 80),
        "recompute": (lambda: bfa.rts_smoother(p, filt_only, out=out), 80 + 80),
        "strided": (lambda: bfa.rts_smoother(p, post, out=out, options={"rts_load_mode": 0}), 160 + 80),
    }
    for mode in args.modes.split(","):
        if mode == "full_cross":
            if out_c is None:
                del out
                torch.cuda.empty_cache()
                out_c = bfa.rts_smoother(p, filt_only, cross_covariances=True)
            fn, bps = (lambda: bfa.rts_smoother(p, filt_only, out=out_c, cross_covariances=True)), 80 + 80 + 64
        else:
            fn, bps = cases[mode]
        sec, reps = timed(fn, args.min_seconds)
        rate = bps * steps / sec
        print(json.dumps({"mode": mode, "B": B, "T": T, "n": n, "ms": round(sec * 1e3, 3), "reps": reps,
                          "steps_per_s": steps / sec, "bytes_per_step": bps, "achieved_TBps": rate / 1e12,
                          "frac_of_8TBps": rate / SPEC_BPS}), flush=True)
    # the pair a user runs: filter emitting the filtered fields only, then the recompute smoother
    del post, filt_only, cases
    out_c = None
    out = None
    torch.cuda.empty_cache()
    fo = bfa.kalman_filter(p, y, initial_means=init, fields=("means", "covariances"))
    so = bfa.rts_smoother(p, fo)

    def pair():
        bfa.kalman_filter(p, y, initial_means=init, fields=("means", "covariances"), out=fo)
        bfa.rts_smoother(p, fo, out=so)
    sec, reps = timed(pair, args.min_seconds)
    print(json.dumps({"mode": "kalman_filter(FILTERED)+rts_smoother(recompute)", "B": B, "T": T, "ms": round(sec * 1e3, 3),
                      "reps": reps, "steps_per_s": steps / sec}), flush=True)


if __name__ == "__main__":
    main()
