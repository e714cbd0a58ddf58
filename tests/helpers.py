"""Seeded synthetic inputs shared by the CPU and GPU tests."""
import os

import numpy as np


def shell_scene(seed, grid=32, cin=28, drop=0.1, batch=0, negative=False):
    """Small plenoxel-like scene: ellipsoid shell in a grid^3 volume, integer coords."""
    rng = np.random.default_rng(seed)
    g = np.arange(grid)
    x, y, z = np.meshgrid(g, g, g, indexing="ij")
    c = (grid - 1) / 2.0
    r = np.sqrt(((x - c) / (0.34 * grid)) ** 2 + ((y - c) / (0.28 * grid)) ** 2 + ((z - c) / (0.31 * grid)) ** 2)
    occ = np.abs(r - 1.0) < 0.12
    occ &= rng.random(occ.shape) > drop
    xyz = np.stack(np.nonzero(occ), 1).astype(np.float32)
    if negative:
        xyz -= grid // 2
    feats = rng.standard_normal((xyz.shape[0], cin)).astype(np.float32)
    return xyz, feats


def batch_scenes(seeds, **kw):
    import torch

    cs, fs = [], []
    for j, s in enumerate(seeds):
        c, f = shell_scene(s, **kw)
        cs.append(np.concatenate([np.full((c.shape[0], 1), j, np.float32), c], 1))
        fs.append(f)
    return torch.from_numpy(np.concatenate(cs)), torch.from_numpy(np.concatenate(fs))


def misaligned(x, requires_grad=False):
    """x [n, C] on the device as a contiguous view that starts 4 bytes into a flat buffer -> (flat leaf, view): C % 4 == 0
    no longer suffices for the 16-byte lanes, so the kernels must take their dword form.  The view is
    flat[1:1 + n * C].view(n, C); with `requires_grad` its gradient arrives in flat.grad at the same place."""
    import torch

    n, C = x.shape
    flat = torch.zeros(n * C + 4, dtype=x.dtype, device="cuda")
    flat[1:1 + n * C] = x.reshape(-1).cuda()
    flat.requires_grad_(requires_grad)
    view = flat[1:1 + n * C].view(n, C)
    assert view.is_contiguous() and view.data_ptr() % 16 == 4
    return flat, view


def class_perm(cls, pad=128):
    """mink_class_partition's form from the class (0..7) of every row: rows grouped by class in row order, every segment
    padded with -1 to a multiple of `pad` (the library's buffer of mink_class_partition_rows entries is this and -1 behind it)."""
    import torch

    segs = []
    for c in range(8):
        rows = torch.nonzero(cls == c).flatten().to(torch.int32)
        segs += [rows, torch.full(((-len(rows)) % pad,), -1, dtype=torch.int32)]
    return torch.cat(segs)


def trunk_node(out):
    """The native-trunk autograd node (minkowski/trunk.py: TrunkFunction) in the graph of `out`, or None when the forward
    pass went module by module.  (`model._trunk_plan` only says the model COULD take the native trunk: a stem too small for
    the streaming weight-gradient kernel -- fewer than ~44 k voxels -- takes the module path.)"""
    seen, stack = set(), [out.grad_fn]
    while stack:
        fn = stack.pop()
        if fn is None or fn in seen:
            continue
        seen.add(fn)
        if hasattr(fn, "saved") and hasattr(fn, "plan"):
            return fn
        stack += [f for f, _ in fn.next_functions]
    return None


def host_threads(cap=16):
    """Cores this process may really use: the scheduler affinity mask capped by the cgroup CPU quota -- never
    os.cpu_count(), which on a shared GPU box reports the machine (128+) while the cgroup grants a fraction: oversubscribed
    BLAS / OpenMP threads made the oracle 12x slower there (BENCH_r03.json cpu_baseline: 128 threads 39.6 k voxels/s, 12
    threads 486.7 k)."""
    try:
        n = len(os.sched_getaffinity(0))
    except (AttributeError, OSError):
        n = os.cpu_count() or 1
    for path in ("/sys/fs/cgroup/cpu.max", "/sys/fs/cgroup/cpu/cpu.cfs_quota_us"):
        try:
            with open(path) as f:
                txt = f.read().split()
            if path.endswith("cpu.max"):
                if txt[0] != "max":
                    n = min(n, max(1, int(int(txt[0]) / int(txt[1]))))
            else:
                quota = int(txt[0])
                with open("/sys/fs/cgroup/cpu/cpu.cfs_period_us") as f:
                    period = int(f.read())
                if quota > 0:
                    n = min(n, max(1, quota // period))
            break
        except (OSError, ValueError, IndexError):
            continue
    return max(1, min(cap, n))


# ---- the bench's training step at full size and what the parity tests read back from it (tests/test_gpu_parity_full.py,
# tests/test_gpu_layerwise.py)
def _baseline_batch(batch=16, grid=128, cin=28):
    from nerf_downstream_amd.co3d_3d.src.data.synthetic import SparseVoxelDataset
    from nerf_downstream_amd.co3d_3d.src.data.utils import collate_mink

    ds = SparseVoxelDataset(phase="train", num_samples=1 << 20, num_classes=51, grid=grid, features=["density", "sh"])
    return collate_mink([ds[i] for i in range(batch)])  # exactly bench.py's first batch


def _bench_like_step(hip, batch, labels, passes=3, before_last_pass=None):
    """The training step exactly as bench.py queues it: flat gradient buffer as the gradient sink of the backward kernels,
    coordinate pyramid launched ahead (defer=True) and finished after the previous pass, map plan replayed on the prepare
    stream (so the shortcut branch forks onto its own stream and the weight gradients run on theirs).  The first pass
    records the plan, the second runs while the third batch's maps are replayed from it (the pyramid of pass p+1 is
    launched before forward p, as in bench.py, so it takes two passes to reach the steady state); gradients and logits
    are those of the LAST pass (train-mode batch norm: neither depends on the
    running statistics that move between passes).  `before_last_pass()`, when given, is called right before the last
    pass's forward (e.g. to snapshot the running statistics that pass moves, or to attach hooks to that pass only); it only
    queues work and never synchronises the device, so the last pass overlaps the tail of the one before as in bench.py."""
    import torch
    import torch.nn.functional as F

    from nerf_downstream_amd.parallel import BucketedGradAllReduce

    reducer = BucketedGradAllReduce(hip)
    tf = hip.process_input(batch)
    out = field = None
    for p in range(passes):
        if p + 1 == passes and before_last_pass is not None:
            before_last_pass()
        nxt = hip.process_input(batch, defer=True) if p + 1 < passes else None
        reducer.zero_grad()
        field = tf
        out = hip(tf)
        F.cross_entropy(out, labels).backward()
        if nxt is not None:
            tf = hip.finish_input(nxt)
        reducer.finish()
    torch.cuda.synchronize()
    return out, field, reducer


def _stem_masks_of_hip_run(out, model):
    """The stem ReLU's branch decisions as the HIP backward kernels take them.  The trunk keeps only the POOLED sum of the
    stem's ReLU output, so its backward kernels recompute z = gamma * xhat + beta from the kept convolution output y and
    the batch's (mean, 1 / std) -- and the two kernels that do so round xhat differently (both are valid fp32):
      * gamma / beta gradients (csrc/batchnorm.hip, colreduce / bn_relu_pool_bwd_kernel; also the forward's own
        decision):                      xhat = fl(fl(y - mean) * invstd),        z = fma(xhat, gamma, beta)
      * the weight gradient (csrc/conv_wgrad.hip, wgrad_stream_kernel<.., FUSE>): xhat = fma(y, invstd, fl(-mean * invstd)), z = fma(xhat, gamma, beta)
    Both are reproduced here in exact fp32 arithmetic on the CPU (an fma through float64: the product of two floats is exact
    there).  -> (mask for bn1.*, mask for conv1.kernel), each [n0, C0] bool."""
    import torch

    node = trunk_node(out)
    x, w0, arena0, nbr0, nbr_pool, i2o, pad, b16, _ = node.saved[0]
    n0, n1, C0 = x.shape[0], nbr_pool.shape[0], w0.shape[-1]
    a = arena0.detach().cpu()
    ny = a.numel() - n1 * C0 - 2 * C0  # floats of the y (+ bf16 input copy) region (minkowski/trunk.py)
    if b16:  # bf16 storage: y is kept as bf16 [n0][C0] at the head of the arena; the kernels widen it and go on in fp32
        y = a[: n0 * C0 // 2].view(torch.bfloat16).view(n0, C0).float()
    else:
        assert ny == n0 * C0
        y = a[: n0 * C0].view(n0, C0)
    mean, invstd = a[ny + n1 * C0 : ny + n1 * C0 + C0], a[ny + n1 * C0 + C0 : ny + n1 * C0 + 2 * C0]
    ga, be = model.bn1.bn.weight.detach().cpu(), model.bn1.bn.bias.detach().cpu()

    def fma(p, q, r):
        return (p.double() * q.double() + r.double()).float()

    xh_bn = (y - mean) * invstd
    xh_w = fma(y, invstd, -mean * invstd)
    return fma(xh_bn, ga, be) > 0, fma(xh_w, ga, be) > 0


def _bf16_operands(storage):
    """oracle.me_cpu.OPERAND_HOOK for BASELINE config #4: every convolution GEMM operand rounded to bf16 (round to nearest even, what
    `(__bf16)v` and the MFMA packers of csrc/conv_common.h / stem16.hip do) exactly where the HIP path rounds it -- forward: rows and
    weights; data gradient: dY and weights, EXCEPT the 1x1x1 strided shortcut, whose data gradient is the exact-fp32 dense GEMM
    mink_dense_xwt (csrc/trunk.hip); weight gradient: rows and dY.  `storage`: the stem's convolution output is also STORED as
    bf16 (set_conv_storage("bf16")): its forward value is rounded, the gradient passes unchanged."""
    import torch

    def rnd(t):
        return t.to(torch.bfloat16).to(t.dtype)

    def hook(t, role, shape):
        K, cin = shape[0], shape[1]
        if role == "fwd_y":
            return rnd(t) if storage and K == 27 and cin <= 32 else t
        if role.startswith("dgrad") and K == 1:
            return t
        return rnd(t)

    return hook
