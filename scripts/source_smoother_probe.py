"""The extended smoother and posterior sampler (S = 4, by key) on Lorenz-63 given as source, next to the registry Lorenz-63
instance of the same build on the same streams and in the same process.  B = 65 536, T = 1 000, reference layout,
observations drawn from the model.  Per measurement: the very first call (the hiprtc build of the source route included), two
warm calls, then device events around each of 7 calls; the median is reported.  The smoother is timed on its default data
path (staged) and on the strided one.  Output: one line per measurement, then the ratios source / registry; pass a file name
to keep it.
Usage: python scripts/source_smoother_probe.py [profiles/source_smoother_probe.txt]
"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bayesianfiltering_amd as bfa  # noqa: E402
from tests import source_smoother_cases as sc  # noqa: E402
nl = bfa.nonlinearities
F32 = np.float32
B, T, S, n = 65536, 1000, 4, 3
m0, Q, R = np.array([1.0, 1.0, 1.0], F32), 1e-2 * np.eye(3, dtype=F32), 0.5 * np.eye(3, dtype=F32)
mk = lambda f: bfa.ParamsNLSSM(m0, np.eye(3, dtype=F32), f, np.zeros(3, F32), Q, nl.linear_emission(np.eye(3, dtype=F32)), np.zeros(3, F32), R)
reg, src = mk(nl.lorenz63()), mk(nl.user_dynamics(sc.L63_SRC, 3, theta=sc.L63_THETA))
rng = np.random.default_rng(0)
x = (m0 + rng.normal(size=(B, 3))).astype(F32)
ys = np.empty((B, T, 3), F32)
s_, r_, b_, dt = (F32(v) for v in sc.L63_THETA)
for t in range(T):   # the Lorenz-63 map on the whole batch
    x0, x1, x2 = x[:, 0], x[:, 1], x[:, 2]
    x = np.stack([dt * s_ * (x1 - x0) + x0, dt * (x0 * r_ - x1 - x0 * x2) + x1, dt * (x0 * x1 - b_ * x2) + x2], axis=1)
    x = (x + F32(0.1) * rng.standard_normal((B, 3), dtype=F32)).astype(F32)
    ys[:, t] = x + F32(np.sqrt(0.5)) * rng.standard_normal((B, 3), dtype=F32)
post = bfa.gaussian_sum_filter(reg, ys, 1, initial_means=np.tile(m0, (B, 1)).reshape(B, 1, 3))
torch.cuda.synchronize()
out = []
def timed(name, fn, reps=7):
    t0 = time.perf_counter(); r = fn(); torch.cuda.synchronize(); first = time.perf_counter() - t0
    r = fn(); torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); r = fn(); b.record(); torch.cuda.synchronize(); ms.append(a.elapsed_time(b))
    med = float(np.median(ms))
    out.append(f"{name}: warm call {first*1e3:.1f} ms, median of {reps} = {med:.3f} ms ({B*T/(med*1e-3):.4g} trajectory-steps/s), all = {[round(x,3) for x in ms]}")
    print(out[-1], flush=True)
    return med, r
res = {}
sm_buf = {}
for tag, p in (("registry", reg), ("source", src)):
    t0 = time.perf_counter(); first = bfa.rts_smoother(p, post); torch.cuda.synchronize()   # allocates (reused below) and builds
    out.append(f"smoother {tag}: very first call (kernel build included) {(time.perf_counter() - t0) * 1e3:.0f} ms")
    res["smoother", tag], r = timed(f"smoother {tag}", lambda: bfa.rts_smoother(p, post, out=first))
    sm_buf[tag] = r.smoothed_means
    del first, r
    torch.cuda.empty_cache()
for tag, p in (("registry", reg), ("source", src)):   # the strided data path on the same streams
    first = bfa.rts_smoother(p, post, options={"rts_load_mode": 0})
    res["strided", tag], r = timed(f"smoother strided path {tag}", lambda: bfa.rts_smoother(p, post, out=first, options={"rts_load_mode": 0}))
    del first, r
    torch.cuda.empty_cache()
key = bfa.PRNGKey(1)
xs = {}
for tag, p in (("registry", reg), ("source", src)):
    t0 = time.perf_counter(); buf = bfa.posterior_sample(p, post, S, key=key); torch.cuda.synchronize()
    out.append(f"sampler {tag}: very first call (kernel build included) {(time.perf_counter() - t0) * 1e3:.0f} ms")
    res["sampler", tag], _ = timed(f"sampler S=4 {tag}", lambda: bfa.posterior_sample(p, post, S, key=key, out=buf))
    xs[tag] = buf[:64].clone()
    del buf
    torch.cuda.empty_cache()
out.append(f"finite streams: {bool(torch.isfinite(post.means).all())}")
out.append(f"ratio source / registry: smoother {res['smoother','source']/res['smoother','registry']:.4f}, strided path {res['strided','source']/res['strided','registry']:.4f}, sampler {res['sampler','source']/res['sampler','registry']:.4f}")
out.append(f"max |source - registry| smoothed means {float((sm_buf['source']-sm_buf['registry']).abs().max()):.3e}, samples {float((xs['source']-xs['registry']).abs().max()):.3e}")
print("\n".join(out))
if len(sys.argv) > 1:
    open(sys.argv[1], "w").write("# scripts/source_smoother_probe.py on one MI355X (gfx950)\n" + "\n".join(out) + "\n")
