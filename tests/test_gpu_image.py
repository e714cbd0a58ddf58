"""GPU: csrc/image.hip against tests/image_restate.py (which tests/test_image_cpu.py holds to Pillow's recorded results).  Every
8-bit result must be EQUAL; the float result must be within 2e-6 absolute: at most eight float32 roundings of values below 4, half
an ulp (2.4e-7) each, about 1e-6, doubled.  The tests read the fixture, never Pillow."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import image_restate as R  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLOAT_TOL = 2e-6


def _images():
    """1x1, 1x7, 5x1, 37x53 (the fixture's, with its black / white / grey / saturated patches), 64x48, a constant 40x30 and
    300x200 (W x H): widths that are no multiple of 4, and in 300x200 several workgroups per histogram."""
    g = np.load(os.path.join(ROOT, "tests", "golden", "augmix_pillow_v1.npz"))
    rng = np.random.default_rng(21)
    big = rng.integers(0, 256, (200, 300, 3), dtype=np.uint8)
    big[..., 1] = 90 + big[..., 1] // 6  # a narrow band: autocontrast stretches, equalize clamps
    big[:60, :80] = (17, 120, 230)  # a constant background patch
    return [g["i0_image"], g["i1_image"], rng.integers(0, 256, (1, 5, 3), dtype=np.uint8), g["i2_image"],
            rng.integers(0, 256, (48, 64, 3), dtype=np.uint8), np.full((30, 40, 3), (9, 200, 77), np.uint8), big]


IMAGES = _images()


def _whole(W, H, S):
    return {"size": (W, H), "S": S, "box": (0, 0, W, H), "target": (S, S), "window": (0, 0)}


def run(images, rows, S, width=3, skew=1, want_stages=True):
    """The C ABI directly: the packed batch `skew` bytes behind a 256-byte boundary.  Returns (out, stages, {(chain, depth): the
    chain's batch as uint8}, the packed bytes as the device holds them after the call)."""
    from nerf_downstream_amd._lib import check, lib

    L = lib()
    dev = torch.device("cuda", 0)
    packed, offsets, sizes = R.pack(images)
    B, n = len(images), packed.size
    raw = torch.zeros(n + 512, dtype=torch.uint8, device=dev)
    start = (-raw.data_ptr()) % 256 + skew
    d_packed = raw[start:start + n]
    d_packed.copy_(torch.from_numpy(packed))
    d_off, d_sz = torch.from_numpy(offsets).to(dev), torch.from_numpy(sizes).to(dev)
    d_prog = torch.from_numpy(np.ascontiguousarray(np.stack(rows), np.float64)).to(dev)
    ws = torch.full((L.mink_img_workspace_bytes(n // 3, B, width, S),), 0x5A, dtype=torch.uint8, device=dev)
    out = torch.full((B, 3, S, S), float("nan"), dtype=torch.float32, device=dev)
    stages = torch.full((B, width + 1, S, S, 3), 0x5A, dtype=torch.uint8, device=dev) if want_stages else None
    for r in range(3):
        check(L.mink_img_chain_round(d_packed.data_ptr(), d_off.data_ptr(), d_sz.data_ptr(), d_prog.data_ptr(), n // 3, B, width, r,
                                     ws.data_ptr(), ws.numel(), None))
    check(L.mink_img_finish(d_packed.data_ptr(), d_off.data_ptr(), d_sz.data_ptr(), d_prog.data_ptr(), n // 3, B, width, S,
                            ws.data_ptr(), ws.numel(), out.data_ptr(), None if stages is None else stages.data_ptr(), None))
    torch.cuda.synchronize()
    bufs = {}
    for i in range(1, width + 1):
        for d in (1, 2, 3):
            o = L.mink_img_chain_buffer_offset(n // 3, B, width, i, d)
            bufs[i, d] = ws[o:o + n].cpu().numpy()
    return out.cpu().numpy(), None if stages is None else stages.cpu().numpy(), bufs, d_packed.cpu().numpy()


def _row(images_index, branches, ws=(0.5, 0.25, 0.25), m=0.375):
    from nerf_downstream_amd.co3d_2d.src.data.transforms import compile_program

    return compile_program({"width": len(branches) - 1, "ws": np.float32(ws[:len(branches) - 1]), "m": np.float32(m),
                            "branches": branches})


def _op(name, p, W, H):
    kind = R.OPS.index(name) + 1
    if name in ("autocontrast", "equalize"):
        return (kind,)
    if name in ("posterize", "solarize"):
        return (kind, p)
    return (kind, *R.op_matrix(name, p, W, H))


OP_SETS = [
    [("autocontrast", None), ("equalize", None), ("posterize", 3)],
    [("solarize", 180), ("rotate", 7), ("rotate", -7)],
    [("shear_x", 0.21), ("shear_x", -0.21), ("shear_y", 0.13)],
    [("shear_y", -0.13), ("translate_x", 5), ("translate_x", -5)],
    [("translate_y", 3), ("translate_y", -3), ("posterize", 4)],
    [("solarize", 253), ("rotate", 0), ("translate_x", 0)],
]


@pytest.mark.parametrize("ops", OP_SETS, ids=lambda ops: "-".join(f"{n}{'' if p is None else p}" for n, p in ops))
def test_every_op_equals_the_restatement(ops):
    S = 7
    rows = []
    for im in IMAGES:
        H, W = im.shape[:2]
        branches = [_whole(W, H, S)]
        for name, p in ops:
            b = _whole(W, H, S)
            b["ops"] = [_op(name, p, W, H)]
            branches.append(b)
        rows.append(_row(0, branches))
    _, _, bufs, packed = run(IMAGES, rows, S)
    ref_packed, offsets, _ = R.pack(IMAGES)
    assert np.array_equal(packed, ref_packed)
    for i, (name, p) in enumerate(ops, 1):
        for b, im in enumerate(IMAGES):
            got = bufs[i, 1][offsets[b]:offsets[b + 1]].reshape(im.shape)
            want = R.apply_op(im, name, p)
            assert np.array_equal(got, want), (name, p, im.shape, int((got != want).sum()))


def test_three_rounds_and_an_untouched_branch():
    """Chains of length 1, 2 and 3 (which chain has which length changes from sample to sample), every round mixing point and
    geometric ops; after the call the chain of depth d lies in buffer (chain, d) and the packed input is as it was."""
    S = 7
    rng = np.random.default_rng(4)
    menu = [("autocontrast", None), ("equalize", None), ("posterize", 3), ("solarize", 200), ("rotate", -4), ("shear_x", 0.1),
            ("shear_y", -0.2), ("translate_x", 2), ("translate_y", -1)]
    rows, plans = [], []
    for b, im in enumerate(IMAGES):
        H, W = im.shape[:2]
        branches, plan = [_whole(W, H, S)], []
        for i in range(3):
            depth = (b + i) % 3 + 1
            ops = [menu[int(rng.integers(0, 9))] for _ in range(depth)]
            br = _whole(W, H, S)
            br["ops"] = [_op(n, p, W, H) for n, p in ops]
            branches.append(br)
            plan.append(ops)
        rows.append(_row(0, branches))
        plans.append(plan)
    out, stages, bufs, packed = run(IMAGES, rows, S)
    ref_packed, offsets, _ = R.pack(IMAGES)
    assert np.array_equal(packed, ref_packed)
    for b, im in enumerate(IMAGES):
        for i, ops in enumerate(plans[b], 1):
            want = im
            for n, p in ops:
                want = R.apply_op(want, n, p)
            got = bufs[i, len(ops)][offsets[b]:offsets[b + 1]].reshape(im.shape)
            assert np.array_equal(got, want), (b, i, ops)
        ref_out, ref_stages, _ = R.run_program(im, rows[b], S)
        assert np.array_equal(stages[b], ref_stages), b
        assert np.abs(out[b] - ref_out).max() <= FLOAT_TOL, b


def _finish_cases(S):
    """(image index, branch description) of the tail's cases."""
    I = R.layout()
    B, Sa, Hu = I["JIT_BRIGHTNESS"], I["JIT_SATURATION"], I["JIT_HUE"]
    orders = [[B, Sa, Hu], [B, Hu, Sa], [Sa, B, Hu], [Sa, Hu, B], [Hu, B, Sa], [Hu, Sa, B]]
    factors = [[0.6, 1.4, 0.4], [1.4, 0.6, -0.4], [0.6, 0.6, -0.4], [1.4, 1.4, 0.4], [0.83, 1.21, 0.137], [1.0, 0.0, 0.0]]
    geo = [
        (6, (100, 50, 5, 5)),  # an upscale
        (6, (20, 10, int(round(3.6 * S)), int(round(3.6 * S))) if 3.6 * S <= 180 else (0, 0, 300, 200)),  # a 3.6x downscale
        (6, (300 - 41, 200 - 23, 41, 23)),  # a box on two borders
        (6, (0, 0, 300, 200)),  # the whole image
        (6, (77, 3, 1, 150)),  # one pixel wide
        (3, (0, 0, 8, 8)),  # black, white, grey and saturated pixels
        (4, (0, 0, 64, 48)), (1, (0, 0, 1, 7)), (0, (0, 0, 1, 1)), (2, (0, 0, 5, 1)), (5, (3, 3, 30, 20)),
    ]
    cases = []
    for n, (idx, box) in enumerate(geo):
        H, W = IMAGES[idx].shape[:2]
        cases.append((idx, {"size": (W, H), "S": S, "box": box, "target": (S, S), "window": (0, 0), "order": orders[n % 6],
                            "factors": factors[n % 6], "flip": bool(n % 2), "rgb": np.float32([0.013, -0.02, 0.007]) * (n % 3)}))
    for idx in (6, 3, 1):  # the centre-crop form: a landscape, a portrait and a 1x7 frame
        H, W = IMAGES[idx].shape[:2]
        box, target, window = R.center_crop_geometry(W, H, S)
        cases.append((idx, {"size": (W, H), "S": S, "box": box, "target": target, "window": window}))
    return cases


@pytest.mark.parametrize("S", [7, 16, 33, 224, 260])
def test_finish_equals_the_restatement(S):
    """S = 260 has two tile columns (the tile is at most 256 wide), S = 224 is the training size; 7, 16 and 33 the cheap ones."""
    cases = _finish_cases(S)
    if S >= 224:
        cases = cases[:4] + cases[5:6] + cases[-3:-2]
    images, rows = [], []
    for n, (idx, br) in enumerate(cases):
        im = IMAGES[idx]
        H, W = im.shape[:2]
        if "order" not in br:  # evaluation: width 0
            rows.append(_row(0, [br], m=0.0))
        else:  # the case as branch 0 and as chain 2 behind an op; other branches take neighbouring cases' parameters
            nxt = cases[(n + 1) % len(cases)]
            other = dict(nxt[1]) if nxt[0] == idx and "order" in nxt[1] else dict(br, flip=not br["flip"])
            b1, b2, b3 = dict(br), dict(other), dict(br, flip=not br["flip"])
            b1["ops"], b2["ops"], b3["ops"] = [_op("posterize", 3, W, H)], [_op("rotate", 5, W, H), _op("solarize", 128, W, H)], []
            rows.append(_row(0, [dict(br), b1, b2, b3], ws=np.float32([0.2, 0.3, 0.5]), m=0.0625 * (n + 1)))
        images.append(im)
    out, stages, _, _ = run(images, rows, S, skew=3)
    out2, stages2, _, _ = run(images, rows, S, skew=3)
    assert np.array_equal(out.view(np.uint32), out2.view(np.uint32)) and np.array_equal(stages, stages2)
    I = R.layout()
    worst = 0.0
    for b, (im, row) in enumerate(zip(images, rows)):
        ref_out, ref_stages, _ = R.run_program(im, row, S)
        k = int(row[I["WIDTH"]]) + 1
        assert np.array_equal(stages[b, :k], ref_stages), (b, cases[b][1]["box"], int((stages[b, :k] != ref_stages).sum()))
        assert (stages[b, k:] == 0x5A).all()
        assert np.isfinite(out[b]).all()
        worst = max(worst, float(np.abs(out[b] - ref_out).max()))
    print(f"S={S}: max |out - restatement| = {worst:.3e}")
    assert worst <= FLOAT_TOL


def test_prepare_image_batch_and_a_sample_that_does_not_fit():
    from nerf_downstream_amd.co3d_2d.src.data.transforms import TRAIN_ORDER, AugMix, Compose, compile_program
    from nerf_downstream_amd.minkowski.utils import prepare_image_batch

    np.random.seed(5)
    gin_S = 16
    recipe = Compose(TRAIN_ORDER)
    for t in recipe.transforms:
        if hasattr(t, "image_size"):
            t.image_size = gin_S
    images = [IMAGES[3], IMAGES[4], IMAGES[6], IMAGES[1]]
    rows = [compile_program(AugMix().draw((im.shape[1], im.shape[0]), recipe.draw)) for im in images]
    packed, offsets, sizes = R.pack(images)
    dev = torch.device("cuda", 0)
    out, stages = prepare_image_batch(torch.from_numpy(packed).to(dev), offsets, sizes, np.stack(rows), size=gin_S, stages=True)
    torch.cuda.synchronize()
    for b, im in enumerate(images):
        ref_out, ref_stages, _ = R.run_program(im, rows[b], gin_S)
        assert np.array_equal(stages[b].cpu().numpy(), ref_stages), b
        assert np.abs(out[b].cpu().numpy() - ref_out).max() <= FLOAT_TOL
    with pytest.raises(ValueError, match="running sum"):
        prepare_image_batch(torch.from_numpy(packed).to(dev), offsets, sizes[::-1].copy(), np.stack(rows), size=gin_S)
    # the C ABI on a program whose box leaves the image: that sample is NaN, its neighbours are computed
    I = R.layout()
    bad = [r.copy() for r in rows]
    bad[1][I["BRANCH"] + I["B_BOX"] + 2] = 10_000
    res, _, _, _ = run(images, bad, gin_S, want_stages=False)
    assert np.isnan(res[1]).all() and np.isfinite(res[0]).all() and np.isfinite(res[2]).all() and np.isfinite(res[3]).all()
