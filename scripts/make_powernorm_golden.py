#!/usr/bin/env python3
"""Record tests/golden/powernorm_ref_v1.npz: the reference's own MaskPowerNorm (co3d_3d/src/models/mink/modules/powernorm.py
of a NeRF-Downstream checkout) run on the CPU in float64 for five training steps and one eval forward, in two configurations:

    a : N = 37, C = 12, group_num = 3, warmup_iters = 2
    b : N = 37, C = 12, group_num = 1, warmup_iters = 2

    python scripts/make_powernorm_golden.py --reference /path/to/NeRF-Downstream

Per step the file holds the input x, the incoming gradient dy, and what the reference made of them: y, dx, dweight, dbias
and, after the step, running_phi, ema_gz and iters; plus the eval input and output and the (non-trivial) weight and bias the
run used.  The fixture is data only: tests/test_powernorm_cpu.py reads it, never the reference tree.

The reference module imports `gin` and `MinkowskiEngine` at the top; neither is needed by MaskPowerNorm, so two empty stand-in
modules go into sys.modules for the import."""
import argparse
import importlib.util
import os
import sys
import types

import numpy as np
import torch

STEPS, N, C, WARMUP = 5, 37, 12, 2
CONFIGS = {"a": 3, "b": 1}  # name -> group_num


def load_reference(root):
    gin = types.ModuleType("gin")
    gin.configurable = lambda *a, **k: (a[0] if a and callable(a[0]) else (lambda f: f))
    me = types.ModuleType("MinkowskiEngine")
    for name in ("MinkowskiBatchNorm", "SparseTensor", "TensorField"):
        setattr(me, name, type(name, (), {}))
    sys.modules.setdefault("gin", gin)
    sys.modules.setdefault("MinkowskiEngine", me)
    path = os.path.join(root, "co3d_3d", "src", "models", "mink", "modules", "powernorm.py")
    spec = importlib.util.spec_from_file_location("reference_powernorm", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def record(mod, group_num, seed):
    g = torch.Generator().manual_seed(seed)
    pn = mod.MaskPowerNorm(C, eps=1e-5, alpha_fwd=0.9, alpha_bkw=0.9, warmup_iters=WARMUP, group_num=group_num).double()
    with torch.no_grad():
        pn.weight.copy_(torch.linspace(0.5, 1.5, C, dtype=torch.float64))
        pn.bias.copy_(torch.linspace(-0.2, 0.2, C, dtype=torch.float64))
    out = {"weight": pn.weight.detach().numpy().copy(), "bias": pn.bias.detach().numpy().copy(),
           "group_num": np.int64(group_num), "warmup_iters": np.int64(WARMUP), "eps": np.float64(1e-5),
           "alpha_fwd": np.float64(0.9), "alpha_bkw": np.float64(0.9)}
    pn.train()
    for step in range(STEPS):
        x = (torch.randn(N, C, generator=g, dtype=torch.float64) * 3 + 1).requires_grad_(True)
        dy = torch.randn(N, C, generator=g, dtype=torch.float64)
        pn.weight.grad = pn.bias.grad = None
        y = pn(x)
        y.backward(dy)
        rec = dict(x=x, dy=dy, y=y, dx=x.grad, dweight=pn.weight.grad, dbias=pn.bias.grad, running_phi=pn.running_phi.reshape(-1),
                   ema_gz=pn.ema_gz.reshape(-1), iters=pn.iters)
        for k, v in rec.items():
            out[f"s{step}_{k}"] = v.detach().numpy().copy()
    pn.eval()
    xe = torch.randn(N, C, generator=g, dtype=torch.float64) * 3 + 1
    with torch.no_grad():
        out["eval_x"], out["eval_y"] = xe.numpy().copy(), pn(xe).numpy().copy()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reference", required=True, help="root of a NeRF-Downstream checkout")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), os.pardir, "tests", "golden",
                                                  "powernorm_ref_v1.npz"))
    args = ap.parse_args()
    mod = load_reference(args.reference)
    data = {"steps": np.int64(STEPS)}
    for i, (name, group_num) in enumerate(CONFIGS.items()):
        for k, v in record(mod, group_num, 20 + i).items():
            data[f"{name}_{k}"] = v
    np.savez_compressed(args.out, **data)
    print(f"wrote {os.path.normpath(args.out)}: {len(data)} arrays, {os.path.getsize(args.out)} bytes")


if __name__ == "__main__":
    main()
