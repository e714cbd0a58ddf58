"""-m gpu: mink_img_paste (csrc/paste.hip) against tests/paste_restate.py, bit for bit over the whole packed batch, on the cases of
tests/golden/bkgd_pillow_v1.npz (scripts/make_bkgd_golden.py names what each is there for); a mixed batch; repeatability; and
`prepare_image_batch(paste=...)` against the same call on frames the restatement composited."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import image_restate as IR  # noqa: E402
import paste_restate as R  # noqa: E402

pytestmark = pytest.mark.gpu

with np.load(os.path.join(ROOT, "tests", "golden", "bkgd_pillow_v1.npz")) as _z:
    GOLDEN = {k: _z[k] for k in _z.files}
NAMES = [str(n) for n in GOLDEN["names"]]


def _case(name):
    return GOLDEN[f"{name}_fg"], GOLDEN[f"{name}_mask"], GOLDEN[f"{name}_bg"], tuple(int(v) for v in GOLDEN[f"{name}_size"])


@pytest.fixture(scope="module")
def restated():
    """The restatement's result of every case, computed once."""
    return {n: R.paste(*_case(n)) for n in NAMES}


def _dev():
    return torch.device("cuda", 0)


def run_paste(bgs, jobs):
    """bgs: the slots' frames; jobs: per sample None or (fg, mask plane, (rw, rh)).  Returns the packed batch after the call."""
    from nerf_downstream_amd._lib import check, lib
    from nerf_downstream_amd.minkowski.utils import image_paste_check

    packed, offsets, sizes = IR.pack(bgs)
    fg, mask, table = R.pack_paste(jobs)
    max_w, max_h = image_paste_check(table, sizes, fg.size, mask.size)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(_dev())  # noqa: E731
    d_packed, d_fg, d_mask = up(packed), up(fg), up(mask)
    d_off, d_sz, d_tab = up(offsets), up(sizes), up(table)
    check(lib().mink_img_paste(d_packed.data_ptr(), d_off.data_ptr(), d_sz.data_ptr(), packed.size // 3, len(bgs), d_fg.data_ptr(),
                               fg.size, d_mask.data_ptr(), mask.size, d_tab.data_ptr(), max_w, max_h,
                               torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return d_packed.cpu().numpy(), offsets


@pytest.mark.parametrize("name", NAMES)
def test_paste_equals_the_restatement(name, restated):
    fg, mask, bg, size = _case(name)
    got, _ = run_paste([bg], [(fg, mask, size)])
    want = restated[name]
    assert np.array_equal(want, GOLDEN[f"{name}_out"])  # (the restatement is Pillow's result: tests/test_paste_cpu.py)
    diff = got.reshape(bg.shape) != want
    assert not diff.any(), (name, int(diff.sum()), np.argwhere(diff)[:5].tolist())


def test_mixed_batch_odd_offsets_and_two_calls(restated):
    """Five slots of odd byte counts, samples 1 and 3 not pasting; frames and masks at odd byte offsets of their buffers too."""
    names = ["p_05000001", None, "all_255", None, "p_0999"]  # 31x29 slots: 2697 bytes each, masks of 899
    fillers = [GOLDEN["p_05_thin_bg"], GOLDEN["one_pixel_bg"]]  # 5x70 and 3x3: 1050 and 27 bytes
    bgs, jobs, want = [], [], []
    for n in names:
        if n is None:
            bgs.append(fillers.pop()), jobs.append(None), want.append(bgs[-1])
        else:
            fg, mask, bg, size = _case(n)
            bgs.append(bg), jobs.append((fg, mask, size)), want.append(restated[n])
    got, offsets = run_paste(bgs, jobs)
    assert [int(o) % 2 for o in offsets[1:4]] == [1, 0, 1]
    table = R.pack_paste(jobs)[2]
    P = R.layout()
    assert table[2, P["FG_OFFSET"]] % 2 == 1 and table[2, P["MASK_OFFSET"]] % 2 == 1 and not table[1].any() and not table[3].any()
    for b, w in enumerate(want):
        assert np.array_equal(got[offsets[b]:offsets[b + 1]], w.reshape(-1)), b
    again, _ = run_paste(bgs, jobs)
    assert np.array_equal(got, again)


def test_prepare_image_batch_with_a_paste(restated):
    """End to end: the paste runs before the chain rounds (equalize reads the histogram of the whole composite), the result is
    bitwise the one of the same call on composited frames, and `packed` holds the composites afterwards."""
    from nerf_downstream_amd.co3d_2d.src.data.transforms import compile_program
    from nerf_downstream_amd.minkowski.utils import prepare_image_batch

    I, S = IR.layout(), 16
    names = ["inside_odd_odd", None, "larger_than_bg"]
    bgs, jobs, comp, rows = [], [], [], []
    for n in names:
        if n is None:
            bgs.append(GOLDEN["p_073_soft_bg"]), jobs.append(None), comp.append(bgs[-1])
        else:
            fg, mask, bg, size = _case(n)
            bgs.append(bg), jobs.append((fg, mask, size)), comp.append(restated[n])
        H, W = bgs[-1].shape[:2]
        base = {"size": (W, H), "S": S, "box": (0, 0, W, H), "target": (S, S), "window": (0, 0), "order": [I["JIT_BRIGHTNESS"]],
                "factors": [1.2, 1.0, 0.0], "flip": False}
        rows.append(compile_program({"width": 1, "ws": np.float32([1.0]), "m": np.float32(0.4),
                                     "branches": [base, dict(base, ops=[(I["OP_EQUALIZE"],)], flip=True)]}))
    rows = np.stack(rows)
    packed, offsets, sizes = IR.pack(bgs)
    fg, mask, table = R.pack_paste(jobs)
    d_packed = torch.from_numpy(packed).to(_dev())
    paste = {"fg": torch.from_numpy(fg).to(_dev()), "mask": torch.from_numpy(mask).to(_dev()), "table": table}
    got = prepare_image_batch(d_packed, offsets, sizes, rows, size=S, paste=paste)
    want = prepare_image_batch(torch.from_numpy(IR.pack(comp)[0]).to(_dev()), offsets, sizes, rows, size=S)
    plain = prepare_image_batch(torch.from_numpy(packed).to(_dev()), offsets, sizes, rows, size=S, paste=None)
    torch.cuda.synchronize()
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    assert not torch.equal(got[0], plain[0]) and torch.equal(got[1].view(torch.int32), plain[1].view(torch.int32))
    assert np.array_equal(d_packed.cpu().numpy(), IR.pack(comp)[0])
    # a table without a pasting sample: nothing is launched, nothing changes
    d_again = torch.from_numpy(packed).to(_dev())
    none = prepare_image_batch(d_again, offsets, sizes, rows, size=S, paste=dict(paste, table=np.zeros_like(table)))
    assert torch.equal(none.view(torch.int32), plain.view(torch.int32)) and np.array_equal(d_again.cpu().numpy(), packed)
    bad = table.copy()
    bad[0, R.layout()["FG_OFFSET"]] = fg.size
    with pytest.raises(ValueError, match="paste table, sample 0"):
        prepare_image_batch(d_again, offsets, sizes, rows, size=S, paste=dict(paste, table=bad))
