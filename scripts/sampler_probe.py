"""Throughput of bf_ffbs_sample_f32 at n = 4, B = 65 536 (the constant-velocity model, reference layout), T sized so that
the outputs fit.

Inputs are the streams the headline Kalman filter writes.  Each case is warmed up, then timed with device events over at
least half a second of work.  Algorithmic bytes per trajectory-step: inputs 160 (full streams) or 80 (recompute), per
sample 16 noise read (noise mode only) + 16 written.  One JSON line per measurement; the smoother's strided and staged
paths on the same inputs for comparison.
Usage: python scripts/sampler_probe.py [--B 65536] [--S 1,8,64] [--spl 0] [--min-seconds 0.5]
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
    ap.add_argument("--S", default="1,8,64")
    ap.add_argument("--spl", default="0", help="comma-separated ffbs_spl values (0 = the library's choice)")
    ap.add_argument("--sample-steps", type=int, default=1 << 27, help="B*S*T per case: T = sample-steps / (B*S), at most 2000")
    ap.add_argument("--min-seconds", type=float, default=0.5)
    ap.add_argument("--smoother", type=int, default=1)
    args = ap.parse_args()
    B, n = args.B, 4
    a = cm.cv_model_arrays()
    p = cm.product_params(a)
    init = np.tile(a["m0"], (B, 1))
    key = bfa.PRNGKey(0)
    for S in (int(s) for s in args.S.split(",")):
        T = int(max(8, min(2000, args.sample_steps // (B * S))))
        y = torch.randn((B, T, 2), device="cuda") * 0.3
        post = bfa.kalman_filter(p, y, initial_means=init, fields=("means", "covariances", "predicted_means", "predicted_covariances"))
        bare = post._replace(predicted_means=None, predicted_covariances=None)
        noise = torch.randn((B, S, T, n), device="cuda")
        out = torch.empty((B, S, T, n), device="cuda")
        for spl in (int(s) for s in args.spl.split(",")):
            opt = {"ffbs_spl": spl} if spl else None
            cases = {
                "noise_full": (lambda: bfa.posterior_sample(p, post, S, noise=noise, out=out, options=opt), 160 + 32 * S),
                "noise_recompute": (lambda: bfa.posterior_sample(p, bare, S, noise=noise, out=out, options=opt), 80 + 32 * S),
                "key_full": (lambda: bfa.posterior_sample(p, post, S, key=key, out=out, options=opt), 160 + 16 * S),
                "key_recompute": (lambda: bfa.posterior_sample(p, bare, S, key=key, out=out, options=opt), 80 + 16 * S),
            }
            for mode, (fn, bps) in cases.items():
                sec, reps = timed(fn, args.min_seconds)
                rate = bps * B * T / sec
                print(json.dumps({"mode": mode, "S": S, "spl": spl, "B": B, "T": T, "n": n, "ms": round(sec * 1e3, 3), "reps": reps,
                                  "sample_steps_per_s": B * T * S / sec, "traj_steps_per_s": B * T / sec, "bytes_per_step": bps,
                                  "achieved_TBps": rate / 1e12, "frac_of_8TBps": rate / SPEC_BPS}), flush=True)
        if args.smoother and S == 1:
            so = bfa.rts_smoother(p, post)
            for mode, o in (("smoother_strided", {"rts_load_mode": 0}), ("smoother_staged", None)):
                sec, reps = timed(lambda: bfa.rts_smoother(p, post, out=so, options=o), args.min_seconds)
                print(json.dumps({"mode": mode, "B": B, "T": T, "n": n, "ms": round(sec * 1e3, 3), "reps": reps,
                                  "traj_steps_per_s": B * T / sec, "bytes_per_step": 240, "achieved_TBps": 240 * B * T / sec / 1e12}),
                      flush=True)
            del so
        del post, bare, noise, out, y
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
