"""-m gpu: mink_img_chain_round / mink_img_finish inside guard bands (tests/guarded.py), by the rules of
tests/test_gpu_guard_rowpass.py: the C ABI directly, every output and the workspace a Guarded of exactly the size
include/mink_hip.h names (the workspace: mink_img_workspace_bytes() to the byte), every input a Guarded.input.  The packed frames
start 1, 2 or 3 bytes behind a 16-byte boundary, so the 16-byte chunks of the chain kernels have scalar heads and tails in every
image; `stages` is given or NULL.  After the call: check() on every buffer, then the values against tests/image_restate.py.
Nothing here is meant to fault."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import image_restate as R  # noqa: E402
from guarded import Guarded, check_all  # noqa: E402

pytestmark = pytest.mark.gpu


def _dev():
    return torch.device("cuda", 0)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _batch(S):
    from nerf_downstream_amd.co3d_2d.src.data.transforms import compile_program

    rng = np.random.default_rng(9)
    shapes = [(1, 1), (7, 1), (1, 5), (53, 37), (30, 40), (70, 90)]  # H, W
    images = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in shapes]
    images[4][:] = (3, 3, 250)  # a constant frame
    menu = [("equalize", None), ("rotate", 6), ("posterize", 3), ("autocontrast", None), ("shear_x", -0.2), ("solarize", 99),
            ("translate_y", 2), ("shear_y", 0.15), ("translate_x", -3)]
    I = R.layout()
    rows = []
    for b, im in enumerate(images):
        H, W = im.shape[:2]
        branches = []
        for k in range(4):
            w, h = max(1, W - k), max(1, H - (k % 2))
            br = {"size": (W, H), "S": S, "box": (W - w, 0, w, h), "target": (S, S), "window": (0, 0), "flip": bool((b + k) % 2),
                  "order": [I["JIT_HUE"], I["JIT_BRIGHTNESS"], I["JIT_SATURATION"]][:k], "factors": [1.3, 0.7, -0.3],
                  "rgb": np.float32([0.01 * k, 0, -0.01])}
            if k:
                ops = [menu[(3 * b + k + r) % 9] for r in range((b + k) % 3 + 1)]
                br["ops"] = [((R.OPS.index(n) + 1,) if p is None else (R.OPS.index(n) + 1, p) if n in ("posterize", "solarize")
                              else (R.OPS.index(n) + 1, *R.op_matrix(n, p, W, H))) for n, p in ops]
            branches.append(br)
        rows.append(compile_program({"width": 3, "ws": np.float32([0.6, 0.3, 0.1]), "m": np.float32(0.7), "branches": branches}))
    return images, np.stack(rows)


@pytest.mark.parametrize("skew,with_stages", [(1, True), (2, False), (3, True)])
def test_image_entry_points_inside_guard_bands(skew, with_stages):
    from nerf_downstream_amd._lib import check, lib

    L, S, width = lib(), 9, 3
    images, rows = _batch(S)
    packed, offsets, sizes = R.pack(images)
    B, n = len(images), packed.size
    gp = Guarded.input(torch.from_numpy(packed).to(_dev()), name="packed", skew=skew)
    assert gp.ptr % 16 == skew
    go = Guarded.input(torch.from_numpy(offsets).to(_dev()), name="offsets")
    gs = Guarded.input(torch.from_numpy(sizes).to(_dev()), name="sizes")
    gr = Guarded.input(torch.from_numpy(rows).to(_dev()), name="programs")
    need = L.mink_img_workspace_bytes(n // 3, B, width, S)
    gw = Guarded(int(need), torch.uint8, _dev(), written="any", name="workspace")
    gout = Guarded((B, 3 * S * S), torch.float32, _dev(), name="out")
    gst = Guarded((B * (width + 1) * S * S * 3,), torch.uint8, _dev(), name="stages") if with_stages else None
    for r in range(3):
        check(L.mink_img_chain_round(gp.ptr, go.ptr, gs.ptr, gr.ptr, n // 3, B, width, r, gw.ptr, need, _stream()))
    check(L.mink_img_finish(gp.ptr, go.ptr, gs.ptr, gr.ptr, n // 3, B, width, S, gw.ptr, need, gout.ptr, gst.ptr if gst else None, _stream()))
    torch.cuda.synchronize()
    if gst is not None:  # (a computed 0x5A byte is not "never written": the mask is every byte that differs from the restatement's 0x5A)
        ref = np.stack([R.run_program(im, row, S)[1] for im, row in zip(images, rows)])
        gst.set_written(torch.from_numpy(ref.reshape(-1) != 0x5A))
    check_all(gp, go, gs, gr, gw, gout, gst)
    out = gout.t.cpu().numpy().reshape(B, 3, S, S)
    for b, (im, row) in enumerate(zip(images, rows)):
        ref_out, ref_stages, _ = R.run_program(im, row, S)
        assert np.abs(out[b] - ref_out).max() <= 2e-6, b
        if gst is not None:
            assert np.array_equal(gst.t.cpu().numpy().reshape(B, width + 1, S, S, 3)[b], ref_stages), b


def test_evaluation_form_needs_no_workspace():
    """width 0 (CenterCrop, out = pre_0): no chain buffers, a NULL workspace and NULL stages are legal."""
    from nerf_downstream_amd._lib import check, lib
    from nerf_downstream_amd.co3d_2d.src.data.transforms import compile_program

    L, S = lib(), 11
    images, _ = _batch(S)
    rows = []
    for im in images:
        H, W = im.shape[:2]
        box, target, window = R.center_crop_geometry(W, H, S)
        rows.append(compile_program({"size": (W, H), "S": S, "box": box, "target": target, "window": window}))
    rows = np.stack(rows)
    packed, offsets, sizes = R.pack(images)
    B, n = len(images), packed.size
    gp = Guarded.input(torch.from_numpy(packed).to(_dev()), name="packed", skew=1)
    go = Guarded.input(torch.from_numpy(offsets).to(_dev()), name="offsets")
    gs = Guarded.input(torch.from_numpy(sizes).to(_dev()), name="sizes")
    gr = Guarded.input(torch.from_numpy(rows).to(_dev()), name="programs")
    gout = Guarded((B, 3 * S * S), torch.float32, _dev(), name="out")
    assert L.mink_img_workspace_bytes(n // 3, B, 0, S) == 0
    check(L.mink_img_chain_round(gp.ptr, go.ptr, gs.ptr, gr.ptr, n // 3, B, 0, 0, None, 0, _stream()))
    check(L.mink_img_finish(gp.ptr, go.ptr, gs.ptr, gr.ptr, n // 3, B, 0, S, None, 0, gout.ptr, None, _stream()))
    torch.cuda.synchronize()
    check_all(gp, go, gs, gr, gout)
    out = gout.t.cpu().numpy().reshape(B, 3, S, S)
    for b, (im, row) in enumerate(zip(images, rows)):
        assert np.array_equal(out[b].view(np.uint32), R.run_program(im, row, S)[0].view(np.uint32)), b
