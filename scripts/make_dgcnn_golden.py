"""Writes tests/golden/dgcnn_knn_v1.npz: inputs of 2 samples x 40 points x 3 channels on a 1/8 lattice and, for k = 20, the
neighbour SETS that the reference's own `knn` (co3d_3d/src/models/mink/dgcnn.py:8-13, loaded by path at run time, run on the
CPU) returns for them.  `topk` leaves the order among equal distances undefined, so only sets are recorded, and the inputs
are drawn until no row has a tie at the k-th boundary; on the lattice every fp32 product and sum of the reference is exact.

    python scripts/make_dgcnn_golden.py --reference /path/to/reference/checkout
"""
import argparse
import importlib.util
import os

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, N, C, K = 2, 40, 3, 20


def draw(seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-64, 65, (B, N, C), generator=g).float() / 8.0


def boundary_tie(x):
    d = ((x[:, :, None, :].double() - x[:, None, :, :].double()) ** 2).sum(-1)
    s = torch.sort(d, dim=2).values
    return bool((s[:, :, K - 1] == s[:, :, K]).any())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="root of the reference checkout")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "dgcnn_knn_v1.npz"))
    args = ap.parse_args()
    spec = importlib.util.spec_from_file_location("ref_dgcnn", os.path.join(args.reference, "co3d_3d", "src", "models", "mink", "dgcnn.py"))
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    seed = 0
    while boundary_tie(draw(seed)):
        seed += 1
    x = draw(seed)
    assert not boundary_tie(x), "a row has a tie at the k-th boundary: topk leaves it undefined"
    idx = ref.knn(x.transpose(2, 1).contiguous(), K)  # the reference's layout is [B, C, N]
    assert idx.shape == (B, N, K)
    sets = np.sort(idx.numpy().astype(np.int16), axis=2)
    assert all(len(set(r.tolist())) == K for r in sets.reshape(-1, K))
    np.savez_compressed(args.out, x=x.numpy(), k=np.int32(K), sets=sets, seed=np.int32(seed))
    print(f"{args.out}: seed {seed}, x {tuple(x.shape)}, sets {sets.shape}")


if __name__ == "__main__":
    main()
