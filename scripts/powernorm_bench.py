#!/usr/bin/env python
"""PowerNorm forward + backward (training mode) in one process with device events, beside

  batch norm        : BatchNormFunction, the kernels MinkowskiBatchNorm runs (csrc/batchnorm.hip) -- what a converted layer ran before
  torch composition : the formulas of tests/pn_restate.py written with torch fp32 operators on the same GPU, the warm-up branch
                      decided the way the reference decides it (`iters.item()`: one host synchronisation per layer and step)

at the stem shape of bench.py (about 826 k rows x 32 channels) and one deep layer shape (13 k rows x 256 channels), with
group_num 1 (the default) and 4, with the fused residual add and ReLU.  Time is the median of ROUNDS x ITERS calls after a
warm-up, peak memory the allocator's high-water mark over one call above what the operands occupy.  No threshold is attached
to either: the feature is correctness and the missing host synchronisation; the numbers are there to be read.

Then the accuracy table: over the shapes and row counts of tests/test_gpu_powernorm.py, the worst ratio of the measured error
to the fp32 bound of tests/pn_restate.py, for the HIP kernels and -- on the same inputs, as the yardstick -- for the torch
composition.

    python scripts/powernorm_bench.py [--out profiles/powernorm_kernels.txt]"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SHAPES = [(826_000, 32), (13_000, 256)]
GROUPS = (1, 4)
WARMUP, ITERS, ROUNDS = 5, 20, 3
EPS, AFWD, ABKW, WARM = 1e-5, 0.9, 0.9, 2


class TorchPowerNorm:
    """The formulas, operator by operator in fp32 (no autograd graph: forward keeps what backward needs)."""

    def __init__(self, C, groups, device):
        self.G = groups
        self.phi, self.ema = torch.ones(C, device=device), torch.zeros(C, device=device)
        self.iters = torch.zeros(1, dtype=torch.int64, device=device)

    def forward(self, x, w, b, res, relu):
        n, C = x.shape
        xg = x.reshape(n, self.G, C // self.G)
        r = torch.rsqrt((xg * xg).mean(2, keepdim=True) + 1e-5)
        xh = (xg * r).reshape(n, C)
        self.iters += 1
        it = int(self.iters.item())  # the reference's host synchronisation
        var = (xh * xh).mean(0)
        s = torch.rsqrt((var if it <= WARM else self.phi) + EPS)
        z = xh * s
        if it < WARM:
            self.phi.copy_(self.phi * (it - 1) / it + var / it)
        self.phi.copy_(AFWD * self.phi + (1 - AFWD) * var)
        y = w * z + b
        if res is not None:
            y = y + res
        if relu:
            y = torch.relu(y)
        self.saved = (r, xh, z, var, y if relu else None)
        return y

    def backward(self, dy, w):
        r, xh, z, var, y = self.saved
        n, C = z.shape
        g0 = torch.where(y > 0, dy, torch.zeros_like(dy)) if y is not None else dy
        a = g0 * w - ((1 - ABKW) * self.ema) * z
        self.ema.add_((a * z).mean(0))
        dxh = a * torch.rsqrt(var + EPS)
        t = (dxh * xh).reshape(n, self.G, -1).mean(2, keepdim=True)
        dx = ((dxh.reshape(n, self.G, -1) - xh.reshape(n, self.G, -1) * t) * r).reshape(n, C)
        return dx, (g0 * z).sum(0), g0.sum(0), g0


def timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / iters  # microseconds


def measure(fn):
    for _ in range(WARMUP):
        fn()
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    ts = [timed(fn, ITERS) for _ in range(ROUNDS)]
    return statistics.median(ts), max(ts) - min(ts), peak / 2 ** 20


def timing_lines(Fn):
    lines = [f"{'rows':>8} {'C':>4} {'G':>2}  {'powernorm us':>12} {'spread':>7} {'MiB':>7}  {'batchnorm us':>12} {'spread':>7} {'MiB':>7}  "
             f"{'torch us':>9} {'spread':>7} {'MiB':>7}  {'GB/s':>6}"]
    for n, C in SHAPES:
        for G in GROUPS:
            x = (torch.randn(n, C, device="cuda") * 3 + 1).requires_grad_(True)
            res = torch.randn(n, C, device="cuda").requires_grad_(True)
            dy = torch.randn(n, C, device="cuda")
            w, b = torch.ones(C, device="cuda", requires_grad=True), torch.zeros(C, device="cuda", requires_grad=True)
            phi, ema = torch.ones(1, C, 1, 1, device="cuda"), torch.zeros(1, C, 1, 1, device="cuda")
            iters = torch.zeros(1, dtype=torch.int64, device="cuda")
            rm, rv = torch.zeros(C, device="cuda"), torch.ones(C, device="cuda")
            tp = TorchPowerNorm(C, G, "cuda")

            def clear():
                for t in (x, res, w, b):
                    t.grad = None

            def pn():
                clear()
                Fn.PowerNormFunction.apply(x, w, b, phi, ema, iters, True, EPS, AFWD, ABKW, WARM, G, res, True).backward(dy)

            def bn():
                clear()
                Fn.BatchNormFunction.apply(x, w, b, rm, rv, True, 0.1, EPS, res, True, None).backward(dy)

            def tc():
                with torch.no_grad():
                    tp.forward(x, w, b, res, True)
                    tp.backward(dy, w)

            (t_pn, s_pn, m_pn), (t_bn, s_bn, m_bn), (t_tc, s_tc, m_tc) = measure(pn), measure(bn), measure(tc)
            # bytes one PowerNorm step has to move: forward reads x three times and the residual once and writes y (20),
            # backward reads dy, x, y in the column pass and again in the group pass and writes dx, dresidual (32)
            gbs = 52.0 * n * C / (t_pn * 1e-6) / 1e9
            lines.append(f"{n:>8} {C:>4} {G:>2}  {t_pn:>12.1f} {s_pn:>7.1f} {m_pn:>7.1f}  {t_bn:>12.1f} {s_bn:>7.1f} {m_bn:>7.1f}  "
                         f"{t_tc:>9.1f} {s_tc:>7.1f} {m_tc:>7.1f}  {gbs:>6.0f}")
    return lines


def accuracy_lines(Fn):
    import pn_restate as PR

    hp = dict(eps=PR.f32(EPS), afwd=PR.f32(AFWD), abkw=PR.f32(ABKW))
    worst = {"hip": {}, "torch": {}}
    for C, G in [(1, 1), (3, 1), (6, 3), (12, 3), (32, 1), (32, 4), (96, 96), (256, 2)]:
        for n in (63, 257, 4099):
            g = torch.Generator().manual_seed(7 + n)
            x, dy, res = torch.randn(n, C, generator=g) * 3 + 1, torch.randn(n, C, generator=g), torch.randn(n, C, generator=g)
            w, b = torch.linspace(0.5, 1.5, C), torch.linspace(-0.2, 0.2, C)
            for it0 in (0, 1, 3):
                phi0 = torch.rand(C, generator=g) * 1.5 + 0.5 if it0 else torch.ones(C)
                ema0 = (torch.rand(C, generator=g) - 0.5) * 0.2 if it0 else torch.zeros(C)
                st = PR.State(phi0, ema0, it0)
                outs = {}
                xs, ws, bs, rs = (t.clone().cuda().requires_grad_(True) for t in (x, w, b, res))
                phi, ema = phi0.clone().reshape(1, C, 1, 1).cuda(), ema0.clone().reshape(1, C, 1, 1).cuda()
                iters = torch.tensor([it0], dtype=torch.int64, device="cuda")
                y = Fn.PowerNormFunction.apply(xs, ws, bs, phi, ema, iters, True, hp["eps"], hp["afwd"], hp["abkw"], WARM, G, rs, True)
                y.backward(dy.cuda())
                outs["hip"] = dict(y=y.detach(), dx=xs.grad, dw=ws.grad, db=bs.grad, phi=phi.reshape(-1), ema=ema.reshape(-1))
                tp = TorchPowerNorm(C, G, "cuda")
                tp.phi.copy_(phi0), tp.ema.copy_(ema0), tp.iters.fill_(it0)
                with torch.no_grad():
                    yt = tp.forward(x.cuda(), w.cuda(), b.cuda(), res.cuda(), True)
                    dxt, dwt, dbt, _ = tp.backward(dy.cuda(), w.cuda())
                outs["torch"] = dict(y=yt, dx=dxt, dw=dwt, db=dbt, phi=tp.phi, ema=tp.ema)
                for path, got in outs.items():
                    yr, aux, mid = PR.forward(x, w, b, st, hp["eps"], hp["afwd"], WARM, G, True, res, True)
                    dx, dw, db, _, after, bw = PR.backward(dy, aux, w, mid, hp["eps"], hp["abkw"], True, got["y"].cpu() > 0)
                    dx_b, dw_b, db_b, ema_b = PR.grad_bounds(aux, bw, w, mid, hp["abkw"], (dx, dw, db, after.ema_gz))
                    ref = dict(y=yr, dx=dx, dw=dw, db=db, phi=after.running_phi, ema=after.ema_gz)
                    bnd = dict(y=PR.forward_bound(aux, yr), dx=dx_b, dw=dw_b, db=db_b, ema=ema_b, phi=PR.phi_bound(aux, st, after, hp["afwd"], WARM))
                    for k in ref:
                        ratio = float(((got[k].cpu().double() - ref[k]).abs() / bnd[k]).max())
                        worst[path][k] = max(worst[path].get(k, 0.0), ratio)
    keys = ("y", "dx", "dw", "db", "phi", "ema")
    lines = ["worst measured error / fp32 bound of tests/pn_restate.py (<= 1 is what tests/test_gpu_powernorm.py asserts of the HIP kernels); "
             "shapes (C, G) of that test, rows 63 / 257 / 4099, iters 0 / 1 / 3 with warmup_iters = 2, residual + ReLU",
             f"{'':>18} " + " ".join(f"{k:>12}" for k in ("y", "dx", "dweight", "dbias", "running_phi", "ema_gz"))]
    for path, name in (("hip", "HIP kernels"), ("torch", "torch fp32 ops")):
        lines.append(f"{name:>18} " + " ".join(f"{worst[path][k]:>12.3f}" for k in keys))
    return lines


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("powernorm_bench measures on the GPU only")
    from nerf_downstream_amd.minkowski import functional as Fn

    lines = [f"device: {torch.cuda.get_device_name(0)}; forward + backward with residual add and ReLU, training mode, microseconds per call, "
             f"median of {ROUNDS} x {ITERS} after {WARMUP} warm-up calls; MiB = peak allocation of one call above its operands; "
             "GB/s = 52 B / element (PowerNorm's own passes) over the PowerNorm time",
             "PowerNorm: 4 + 3 launches, no host synchronisation; torch composition: the warm-up branch reads iters back every call"]
    lines += timing_lines(Fn)
    lines += accuracy_lines(Fn)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
