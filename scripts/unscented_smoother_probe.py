"""Throughput of bf_uks_smoother_f32 and bf_uffbs_sample_f32 next to the extended entry points on the same streams.

Per state dimension one model (n = 3 Lorenz-63 with every state observed, n = 4 manoeuvring target + bearing / range with inputs,
n = 8, 12, 24 Lorenz-96 + even-state emission), observations drawn from the model on the device, streams from the unscented
filter with ParamsUKF(1, 0, 0).  B = 65 536 for n <= 8, 8 192 at n = 12, 2 048 at n = 24; T = 1 000; the sampler draws S = 4 by
key.  Each call is warmed up once, then timed with device events over at least --min-seconds of work.  One JSON line per
measurement, then the ratio of the unscented to the extended route.
Usage: python scripts/unscented_smoother_probe.py [--n 3,4,8,12,24] [--T 1000] [--B 0] [--S 4] [--min-seconds 0.5]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bayesianfiltering_amd as bfa  # noqa: E402
from bayesianfiltering_amd import random as bfr  # noqa: E402

F32 = np.float32


def timed(fn, min_seconds, warmup=1):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    once = e0.elapsed_time(e1) / 1e3
    if once >= min_seconds:
        return once, 1
    reps = max(1, int(np.ceil(min_seconds / max(once, 1e-6))))
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / 1e3 / reps, reps


def model(n, T):
    nl = bfa.nonlinearities
    u = None
    if n == 3:
        # (every state observed: under the quadratic emission alone the filter does not stay finite over 1 000 steps)
        f, h, m = nl.lorenz63(), nl.linear_emission(np.eye(3, dtype=F32)), 3
        m0, P0, Q, R = np.array([0.0, 1.0, 1.05], F32), np.eye(3, dtype=F32), 0.1 * np.eye(3, dtype=F32), 0.5 * np.eye(3, dtype=F32)
    elif n == 4:
        f, h, m = nl.maneuver_bot(), nl.bearing_range(), 2
        m0, P0 = np.array([2.0, 0.3, 3.0, -0.2], F32), np.diag([0.1, 0.005, 0.1, 0.01]).astype(F32)
        Q, R = 1e-3 * np.eye(2, dtype=F32), np.diag([1e-3, 1e-2]).astype(F32)
        u = (np.arange(T) // 8 % 3).astype(F32)
    else:
        f, h, m = nl.lorenz96(n), nl.pick_even(n), n // 2
        m0, P0, Q, R = np.zeros(n, F32), np.eye(n, dtype=F32), 1e-2 * np.eye(n, dtype=F32), 1e-1 * np.eye(m, dtype=F32)
    dq = Q.shape[0]
    p = bfa.ParamsNLSSM(m0, P0, f, np.zeros(dq, F32), Q, h, np.zeros(m, F32), R)
    return p, (n, dq, m, m), u


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", default="3,4,8,12,24")
    ap.add_argument("--T", type=int, default=1000)
    ap.add_argument("--B", type=int, default=0, help="0: 65 536 for n <= 8, 8 192 at n = 12, 2 048 above")
    ap.add_argument("--S", type=int, default=4)
    ap.add_argument("--min-seconds", type=float, default=0.5)
    args = ap.parse_args()
    up = bfa.ParamsUKF(1.0, 0.0, 0.0)
    key = bfa.PRNGKey(0)
    T, S = args.T, args.S
    for n in (int(v) for v in args.n.split(",")):
        B = args.B or (65536 if n <= 8 else (8192 if n == 12 else 2048))
        p, dims, u = model(n, T)
        keys = bfr.split(bfa.PRNGKey(n), B)
        y = bfa.NonlinearSSM(*dims).sample(p, keys, T, u)[1] if u is not None else bfa.NonlinearSSM(*dims).sample(p, keys, T)[1]
        init = np.tile(np.asarray(p.initial_mean, F32), (B, 1)).reshape(B, 1, n)
        post = bfa.unscented_gaussian_sum_filter(p, up, y, 1, 1, u, initial_means=init)
        finite = bool(torch.isfinite(post.predicted_covariances).all())
        so = bfa.rts_smoother(p, post, inputs=u, extended=True)
        xo = torch.empty((B, S, T, n), device="cuda")
        cases = {
            "eks_smoother": lambda: bfa.rts_smoother(p, post, inputs=u, extended=True, out=so),
            "uks_smoother": lambda: bfa.rts_smoother(p, post, inputs=u, uparams=up, out=so),
            "effbs_sample": lambda: bfa.posterior_sample(p, post, S, key=key, inputs=u, extended=True, out=xo),
            "uffbs_sample": lambda: bfa.posterior_sample(p, post, S, key=key, inputs=u, uparams=up, out=xo),
        }
        rate = {}
        for mode, fn in cases.items():
            sec, reps = timed(fn, args.min_seconds)
            rate[mode] = B * T / sec
            print(json.dumps({"mode": mode, "n": n, "B": B, "T": T, "S": S if "sample" in mode else None, "streams_finite": finite,
                              "ms": round(sec * 1e3, 3), "reps": reps, "traj_steps_per_s": B * T / sec}), flush=True)
        print(json.dumps({"n": n, "uks_over_eks": rate["uks_smoother"] / rate["eks_smoother"],
                          "uffbs_over_effbs": rate["uffbs_sample"] / rate["effbs_sample"]}), flush=True)
        del post, so, xo, y, cases
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
