"""Times farthest-point sampling of a batch of scenes (csrc/sample.hip mink_fps_scenes through minkowski/utils.py
farthest_point_sample) beside the same loop written with torch operations on the same GPU -- the reference's algorithm
(transforms.py:603-626) moved to the device unchanged, one scene after the other -- and one training step of
configs/co3d_points.gin + dgcnn.gin with the sampler running on the prepare stream against the same step on scenes that
were cut down beforehand.

    python scripts/fps_bench.py [--out profiles/fps_kernels.txt] [--repeats 5]

  shape    : the bench's batch: 16 synthetic plenoxel scenes on a 128^3 grid (about 51.6 k voxels each, about 825 k per batch),
             num_points in {1024, 2048}
  kernel   : device-event time of `farthest_point_sample` alone (status word not read back), and of the torch loop; the two
             alternate window by window; their picks are compared
  step     : host clock around windows of pipelined steps that end synchronised (the trainer's loop: batch i + 1 goes through
             process_input(defer=True) while batch i is in forward and backward), DGCNN_cls on 16 x 1024 points; and
             process_input alone, synchronised, for the share of the step that is preparation

Every figure is the median [min .. max] over `--repeats` windows after a warm-up of the same shape.  Needs the GPU: there is no
CPU path."""
import argparse
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from dgcnn_bench import time_windows  # noqa: E402

from nerf_downstream_amd import gin_lite as gin  # noqa: E402
from nerf_downstream_amd.minkowski.utils import farthest_point_sample  # noqa: E402

CFG = os.path.join(ROOT, "nerf_downstream_amd", "co3d_3d", "configs")


def torch_fps(xyz, offsets, m, start):
    """The reference's loop with device tensors, scene by scene: nothing comes back to the host inside it."""
    out = []
    for b in range(len(offsets) - 1):
        p = xyz[offsets[b]:offsets[b + 1]]
        centroids = torch.zeros(m, dtype=torch.long, device=p.device)
        distance = torch.ones(p.shape[0], device=p.device) * 1e10
        farthest = torch.tensor(start[b], device=p.device)
        for i in range(m):
            centroids[i] = farthest
            dist = torch.sum((p - p[farthest]) ** 2, -1)
            mask = dist < distance
            distance[mask] = dist[mask]
            farthest = torch.argmax(distance, -1)
        out.append(centroids + offsets[b])
    return torch.stack(out)


def scenes(batch, grid):
    from nerf_downstream_amd.co3d_3d.src.data.synthetic import SparseVoxelDataset

    ds = SparseVoxelDataset(phase="train", num_samples=1 << 20, num_classes=51, grid=grid, features=["sh"])
    return [ds[i]["coordinates"] for i in range(batch)]


def write_tree(root, coords, grid):
    rng = np.random.default_rng(0)
    os.makedirs(os.path.join(root, "filelist"))
    lines = []
    for j, c in enumerate(coords):
        c = c.numpy().astype(np.int64)
        links = np.sort(c[:, 0] * grid * grid + c[:, 1] * grid + c[:, 2]).astype(np.int32)
        scene = os.path.join(root, "data", f"plenoxel_co3d_s{j}")
        os.makedirs(scene)
        np.savez(os.path.join(scene, "data.npz"), links=links, density=rng.random((len(links), 1)).astype(np.float32),
                 sh=rng.integers(0, 256, (len(links), 27)).astype(np.uint8), sh_min=np.float32(-1.5), sh_scale=np.float32(0.0123))
        lines.append(f"cup s{j}")
    for f in ("train.txt", "test.txt"):
        open(os.path.join(root, "filelist", f), "w").write("\n".join(lines) + "\n")


def step_windows(net, opt, variants, repeats, steps):
    """ms per step of every variant (a list of device batches each), the variants alternating window by window."""
    def run(batches, n):
        field = net.process_input(batches[0])
        for i in range(n):
            nxt = net.process_input(batches[(i + 1) % len(batches)], defer=True)
            opt.zero_grad(set_to_none=True)
            loss = torch.nn.functional.cross_entropy(net(field), batches[i % len(batches)]["labels"])
            loss.backward()
            field = net.finish_input(nxt)
            opt.step()
        torch.cuda.synchronize()

    out = [[] for _ in variants]
    for v in variants:
        run(v, 5)
    for _ in range(repeats):
        for k, v in enumerate(variants):
            t = time.perf_counter()
            run(v, steps)
            out[k].append((time.perf_counter() - t) / steps * 1e3)
    return [(statistics.median(v), min(v), max(v)) for v in out]


def prepare_windows(net, variants, repeats, calls):
    """ms per process_input call alone (decode, sampler, augmentation, field and maps; nothing else on the GPU), synchronised."""
    out = [[] for _ in variants]
    for _ in range(repeats + 1):  # (the first round warms up)
        for k, v in enumerate(variants):
            torch.cuda.synchronize()
            t = time.perf_counter()
            for i in range(calls):
                net.process_input(v[i % len(v)])
            torch.cuda.synchronize()
            out[k].append((time.perf_counter() - t) / calls * 1e3)
    return [(statistics.median(v[1:]), min(v[1:]), max(v[1:])) for v in out]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--grid", type=int, default=128)
    ap.add_argument("--steps", type=int, default=20)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "fps_bench needs the GPU"
    dev = torch.device("cuda")
    coords = scenes(args.batch, args.grid)
    sizes = [int(c.shape[0]) for c in coords]
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    xyz, offsets = torch.cat(coords).to(dev), torch.tensor(off, dtype=torch.int32, device=dev)
    start = [n // 2 for n in sizes]
    first = torch.tensor(start, dtype=torch.int32, device=dev)
    fmt = lambda t: f"{t[0]:9.3f} [{t[1]:.3f} .. {t[2]:.3f}] ms"  # noqa: E731
    lines = [f"fps_bench: mink_fps_scenes vs the reference's loop in torch operations, fp32, {torch.cuda.get_device_name(0)}",
             f"{args.batch} scenes of {min(sizes)} .. {max(sizes)} voxels ({off[-1]} per batch); median [min .. max] per call over "
             f"{args.repeats} windows", ""]
    for m in (1024, 2048):
        fns = [lambda: farthest_point_sample(xyz, offsets, m, first, n_max=max(sizes), status_async=True),
               lambda: torch_fps(xyz, off.tolist(), m, start)]
        hip, ref = time_windows(fns, args.repeats)
        same = float((fns[0]()[0] == fns[1]()).float().mean())
        lines.append(f"num_points {m:4d}: mink_fps_scenes {fmt(hip)} | torch loop {fmt(ref)} | ratio {ref[0] / hip[0]:.1f}x | "
                     f"{hip[0] * 1e3 / m:.2f} us per pick of the batch | same picks {same:.5f}")
    lines.append("")

    from nerf_downstream_amd.co3d_3d.src.data.co3d import Co3DDataset
    from nerf_downstream_amd.co3d_3d.src.data.utils import collate_mink
    from nerf_downstream_amd.co3d_3d.src.models import get_model

    with tempfile.TemporaryDirectory() as tmp:
        write_tree(tmp, coords, args.grid)
        cwd = os.getcwd()
        os.chdir(tmp)
        try:
            gin.clear_config()
            gin.parse_config_files_and_bindings([f"{CFG}/co3d_cls.gin", f"{CFG}/co3d_points.gin", f"{CFG}/dgcnn.gin"],
                                                [f"Co3DDatasetBase.data_root='{tmp}/data'"])
            ds = Co3DDataset(phase="train", compact=True)
            m = ds.sampler.num_points
            hosts = [collate_mink([ds[i] for i in range(args.batch)]) for _ in range(2)]
            to_dev = lambda h: {k: (v.to(dev) if torch.is_tensor(v) and k != "aug_params" else v) for k, v in h.items()}  # noqa: E731
            sampled = [to_dev(h) for h in hosts]
            cut = []  # the same scenes cut down beforehand: no sampler stage in process_input
            for b in sampled:
                xyz_b = torch.stack([b["links"] // (128 * 128), b["links"] % (128 * 128) // 128, b["links"] % 128], 1).float()
                rows = farthest_point_sample(xyz_b, b["scene_offsets"], m, b["fps_start"]).reshape(-1)
                drop = ("fps_start", "sample_points", "sample_n_max")
                d = {k: v for k, v in b.items() if k not in drop}
                d.update(links=b["links"][rows], density=b["density"][rows], sh_q=b["sh_q"][rows],
                         scene_offsets=torch.arange(args.batch + 1, dtype=torch.int32, device=dev) * m)
                cut.append(d)
            from nerf_downstream_amd.memory import reserve

            reserve(dev)  # (as train.py: one segment for the caching allocator, no hipMalloc inside the windows)
            torch.manual_seed(0)
            net = get_model().cuda().train()
            opt = torch.optim.SGD(net.parameters(), lr=0.01, momentum=0.9)
            with_s, without = step_windows(net, opt, [sampled, cut], args.repeats, args.steps)
            prep_s, prep_c = prepare_windows(net, [sampled, cut], args.repeats, 10)
        finally:
            os.chdir(cwd)
            gin.clear_config()
    lines += [f"one training step of co3d_points.gin + dgcnn.gin ({type(net).__name__}, {args.batch} x {m} points), pipelined as in train.py, "
              f"windows of {args.steps} steps:",
              f"  FarthestPointSample on the prepare stream {fmt(with_s)}",
              f"  scenes cut down beforehand (no sampler)    {fmt(without)}",
              f"  difference {with_s[0] - without[0]:+.3f} ms per step",
              "process_input alone (decode, sampler, augmentation, field; nothing beside it on the GPU), per call:",
              f"  with FarthestPointSample                   {fmt(prep_s)}",
              f"  scenes cut down beforehand                 {fmt(prep_c)}"]
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
