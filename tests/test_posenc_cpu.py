"""CPU: the positional encoding and the networks built on it, without a GPU -- the float64 restatement of
tests/posenc_restate.py against an independent dense-matrix form under torch autograd, the module's state dict (the
reference's three non-trainable parameters), the registry with the five *Ins and the two Encoded* classes and their state-dict
keys (tests/golden/encoded_unet_state_keys_v1.json), the new config, the C ABI's argument checks (every one before the first
launch) and the refusal of an INSSEG model by the segmentation trainer."""
import json
import math
import os

import pytest
import torch

import posenc_restate as R
from nerf_downstream_amd import _lib
from nerf_downstream_amd import gin_lite as gin

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, "nerf_downstream_amd", "co3d_3d", "configs")
CASES = [(3, 4, None), (3, 6, (0, 3)), (28, 4, None), (5, 0, None)]


@pytest.fixture(autouse=True)
def _clean_gin():
    gin.clear_config()
    yield
    gin.clear_config()


def _dense_form(x, C, L, min_resolution=None):
    """The second form: x [n, C] @ M [C, Q] + phase, then sin; M[c, q] = f[q mod L] where c == q // (2L).  Built with tensor
    ops, not with the restatement's helpers."""
    Q = 2 * L * C
    if min_resolution is None:
        f = 2.0 ** torch.arange(L, dtype=torch.float64)
    else:
        m = math.log2(0.5 / min_resolution)
        f = 2.0 ** torch.linspace(m - L - 1, m, L, dtype=torch.float64)
    q = torch.arange(Q)
    M = torch.zeros(C, Q, dtype=torch.float64)
    M[q // (2 * L), q] = f.repeat(2 * C)
    phase = torch.cat([torch.zeros(C * L, dtype=torch.float64), torch.full((C * L,), math.pi / 2, dtype=torch.float64)])
    return torch.sin(x @ M + phase)


@pytest.mark.parametrize("C,L,rng,res", [(1, 1, None, None), (3, 4, None, None), (3, 6, (0, 3), None), (5, 3, (1, 2), None),
                                         (28, 4, None, None), (3, 6, None, 0.01), (4, 1, (2, 4), 0.25)])
def test_restatement_equals_dense_form_and_autograd(C, L, rng, res):
    g = torch.Generator().manual_seed(C * 100 + L)
    x = (1.5 * torch.randn(37, C, generator=g, dtype=torch.float64)).requires_grad_(True)
    chan, freq, phase = R.columns(C, L, res)
    lo, hi = rng or (0, 0)
    want = torch.cat([_dense_form(x, C, L, res), x[:, lo:hi]], dim=1)
    got = R.forward(x.detach(), chan, freq, phase, rng)
    assert got.shape == (37, 2 * L * C + hi - lo)
    assert float((got - want.detach()).abs().max()) <= 1e-12
    dy = torch.randn(want.shape, generator=g, dtype=torch.float64)
    (dx,) = torch.autograd.grad(want, x, dy)
    got_dx = R.backward(x.detach(), dy, chan, freq, phase, rng)
    assert float((got_dx - dx).abs().max()) <= 1e-10 * float(freq.max())
    # the column-index phase split: channels of the first half hold their L sines twice, those of the second half cosines twice
    if C >= 2 and res is None:
        first, last = got[:, : 2 * L], got[:, 2 * L * (C - 1): 2 * L * C]
        assert torch.equal(first[:, :L], first[:, L:]) and torch.equal(last[:, :L], last[:, L:])
        xs = x.detach()
        assert float((first[:, 1] - torch.sin(2 * xs[:, 0])).abs().max()) <= 1e-12 if L > 1 else True
        assert float((last[:, 0] - torch.cos(xs[:, C - 1])).abs().max()) <= 1e-12


def test_min_resolution_frequencies_span_l_plus_one_octaves():
    f = R.base_frequencies(6, 0.01)
    assert f[-1].item() == pytest.approx(50.0, rel=1e-12) and f[0].item() == pytest.approx(50.0 / 2 ** 7, rel=1e-12)
    assert torch.allclose(f[1:] / f[:-1], torch.full((5,), 2.0 ** (7 / 5), dtype=torch.float64), rtol=1e-12)


@pytest.mark.parametrize("C,L,rng", CASES)
def test_module_state_dict_and_out_channels(C, L, rng):
    from nerf_downstream_amd import minkowski as ME

    enc = ME.MinkowskiPositionalEncoding(C, num_encoding_functions=L, include_original_channel_range=rng)
    sd = enc.state_dict()
    if L < 1:
        assert len(sd) == 0 and enc.out_channels == C and list(enc.parameters()) == []
        return
    Q = 2 * L * C
    assert enc.out_channels == Q + (rng[1] - rng[0] if rng else 0)
    assert list(sd) == ["coo", "frequencies", "offset"]  # the reference's three, in its order; no `mat`
    assert (sd["coo"].shape, sd["coo"].dtype) == ((2, Q), torch.int64)
    assert (sd["frequencies"].shape, sd["frequencies"].dtype) == ((Q,), torch.float32)
    assert (sd["offset"].shape, sd["offset"].dtype) == ((1, Q), torch.float32)
    assert not any(p.requires_grad for p in enc.parameters()) and len(list(enc.buffers())) == 0
    chan, freq, phase = R.columns(C, L)
    assert torch.equal(sd["coo"][0], chan) and torch.equal(sd["coo"][1], torch.arange(Q))
    assert torch.equal(sd["frequencies"].double(), freq)  # powers of two: exact
    assert torch.equal(sd["offset"].view(-1), phase.float())
    # round trip: a checkpoint's values rule
    other = ME.MinkowskiPositionalEncoding(C, num_encoding_functions=L, include_original_channel_range=rng)
    changed = {"coo": sd["coo"].clone(), "frequencies": sd["frequencies"] * 3, "offset": sd["offset"] + 0.25}
    other.load_state_dict(changed)
    assert torch.equal(other.frequencies, changed["frequencies"]) and torch.equal(other.offset, changed["offset"])
    assert not other.frequencies.requires_grad and not other.offset.requires_grad


def test_module_min_resolution_and_checks():
    from nerf_downstream_amd import minkowski as ME

    enc = ME.MinkowskiPositionalEncoding(3, 6, None, 0.01)
    want = R.base_frequencies(6, 0.01)
    got = enc.frequencies.detach().double()
    assert torch.allclose(got[:6], want, rtol=4e-6) and torch.equal(got, got[:6].repeat(6))  # fp32 linspace and exp2
    assert got[5].item() == pytest.approx(50.0, rel=1e-6) and got[0].item() == pytest.approx(0.390625, rel=4e-6)
    with pytest.raises(ValueError, match="include_original_channel_range"):
        ME.MinkowskiPositionalEncoding(3, 4, (2, 4))
    with pytest.raises(ValueError, match="min_resolution"):
        ME.MinkowskiPositionalEncoding(3, 4, None, "0.01")
    gin.parse_config(["MinkowskiPositionalEncoding.num_encoding_functions = 2"])
    assert ME.MinkowskiPositionalEncoding(3).out_channels == 12
    from nerf_downstream_amd import install_as_minkowski_engine

    assert install_as_minkowski_engine().MinkowskiPositionalEncoding is ME.MinkowskiPositionalEncoding
    from nerf_downstream_amd.minkowski.functional import PositionalEncodingFunction  # noqa: F401


def test_tensorfield_sparse_takes_the_quantization_mode():
    import inspect

    from nerf_downstream_amd import minkowski as ME
    from nerf_downstream_amd.minkowski import tensor as T

    assert "quantization_mode" in inspect.signature(ME.TensorField.sparse).parameters
    T._check_quantization_mode("TensorField.sparse", None)
    T._check_quantization_mode("TensorField.sparse", ME.SparseTensorQuantizationMode.UNWEIGHTED_AVERAGE)
    with pytest.raises(NotImplementedError, match="UNWEIGHTED_AVERAGE"):
        T._check_quantization_mode("TensorField.sparse", ME.SparseTensorQuantizationMode.RANDOM_SUBSAMPLE)


INS = ["Res16UNet14AIns", "Res16UNet14BIns", "Res16UNet18AIns", "Res16UNet18BIns", "Res16UNet34CIns"]
OFFSET_KEYS = ["offset_block.0.kernel", "offset_block.0.bias", "offset_block.1.bn.weight", "offset_block.1.bn.bias",
               "offset_block.1.bn.running_mean", "offset_block.1.bn.running_var", "offset_block.1.bn.num_batches_tracked",
               "offset_block.3.kernel", "offset_block.3.bias"]
ENCODED_KEYS = ["final.linear.weight", "final.linear.bias", "encoding.coo", "encoding.frequencies", "encoding.offset",
                "enc_mlp.0.0.linear.weight", "enc_mlp.0.0.linear.bias", "enc_mlp.1.0.linear.weight", "enc_mlp.1.0.linear.bias",
                "dec_mlp.0.0.linear.weight", "dec_mlp.0.0.linear.bias", "dec_mlp.1.0.linear.weight", "dec_mlp.1.0.linear.bias"]


def test_registry_and_state_dict_keys():
    from nerf_downstream_amd.co3d_3d.src.models import MODELS, get_model
    from nerf_downstream_amd.co3d_3d.src.models.mink import res16unet as U

    for name in INS + ["EncodedRes16UNet", "EncodedRes16UNet2"]:
        assert name in MODELS and MODELS[name] is getattr(U, name), name
    for name in INS:
        assert MODELS[name].INSSEG and not MODELS[name[:-3]].INSSEG and issubclass(MODELS[name], MODELS[name[:-3]])
    with open(os.path.join(ROOT, "tests", "golden", "encoded_unet_state_keys_v1.json")) as f:
        golden = json.load(f)

    torch.manual_seed(0)
    ins = get_model("Res16UNet14AIns", 3, 20)
    got = [[k, list(v.shape)] for k, v in ins.state_dict().items()]
    assert got == golden["Res16UNet14AIns"] and len(got) == 209
    plain = list(get_model("Res16UNet14A", 3, 20).state_dict())
    assert [k for k, _ in got] == plain + OFFSET_KEYS  # the plain network's keys, then the head's
    sd = ins.state_dict()
    assert tuple(sd["offset_block.0.kernel"].shape) == (96, 96) and tuple(sd["offset_block.0.bias"].shape) == (1, 96)
    assert tuple(sd["offset_block.3.kernel"].shape) == (96, 3) and tuple(sd["offset_block.3.bias"].shape) == (1, 3)
    assert tuple(sd["offset_block.1.bn.weight"].shape) == (96,)

    enc = get_model("EncodedRes16UNet", 3, 20)
    got = [[k, list(v.shape)] for k, v in enc.state_dict().items()]
    assert got == golden["EncodedRes16UNet"] and len(got) == 307
    unet = [k for k in get_model("Res16UNet", 32, 20).state_dict() if k not in ("final.kernel", "final.bias")]
    assert [k for k, _ in got] == unet + ENCODED_KEYS and "final.kernel" not in enc.state_dict()
    assert tuple(enc.conv0p1s1[0].kernel.shape) == (27, 32, 32)  # the U is built on ENC_PLANES[-1] channels
    assert enc.encoding.out_channels == 24 and enc.enc_mlp[0][0].linear.weight.shape == (32, 24)
    assert enc.dec_mlp[0][0].linear.weight.shape[1] == 96 and tuple(enc.final.linear.weight.shape) == (20, 48)
    enc2 = get_model("EncodedRes16UNet2", 3, 20)
    assert list(enc2.state_dict()) == list(enc.state_dict())
    assert enc2.dec_mlp[0][0].linear.weight.shape[1] == 88
    wide = U.EncodedRes16UNet(5, 7, ENC_PLANES=(16, 24, 40), DEC_PLANES=(12,))
    assert wide.conv0p1s1[0].kernel.shape[1] == 40 and len(wide.enc_mlp) == 3 and len(wide.dec_mlp) == 1
    assert wide.dec_mlp[0][0].linear.weight.shape == (12, 64 + 40) and wide.final.linear.weight.shape == (7, 12)
    # the encoding's tensors never train
    assert not any(p.requires_grad for p in enc.encoding.parameters())


@pytest.mark.parametrize("base", ["scannet_plenoxel.gin", "scannet_semseg.gin", "synthetic_seg.gin"])
def test_config_parses_and_resolves(base):
    from nerf_downstream_amd.co3d_3d.src.models import get_model
    import nerf_downstream_amd.co3d_3d.train  # noqa: F401  (registers the configurables the base files bind)

    gin.parse_config_files_and_bindings([os.path.join(CFG, base), os.path.join(CFG, "encoded_res16unet.gin")], [], skip_unknown=True)
    assert gin.query_parameter("get_model.name") == "EncodedRes16UNet"
    assert gin.query_parameter("EncodedRes16UNet.ENC_PLANES") == (32, 32) and gin.query_parameter("EncodedRes16UNet.DEC_PLANES") == (48, 48)
    gin.parse_config(["EncodedRes16UNet.DEC_PLANES = (40, 24)"])
    m = get_model(in_channel=4, out_channel=6)
    assert type(m).__name__ == "EncodedRes16UNet" and m.final.linear.weight.shape == (6, 24) and m.encoding.out_channels == 32


def test_signatures():
    S = _lib.SIGNATURES
    assert "mink_posenc_fwd" in S and "mink_posenc_bwd" in S
    assert len(S["mink_posenc_fwd"][1]) == 12 and len(S["mink_posenc_bwd"][1]) == 14
    assert _lib.CONSTANTS["MINK_ABI_VERSION"] == 4  # additive change


def test_argument_validation_without_gpu():
    """Every check of mink_posenc_fwd / _bwd comes before the first launch."""
    L = _lib.lib()
    P = 0x10000  # aligned, never dereferenced
    fwd = dict(x=P, n=10, C=3, ldx=3, freq=P, phase=P, L=4, lo=0, hi=3, y=P, ldy=27, stream=None)
    bwd = dict(dy=P, ldy=27, x=P, n=10, C=3, ldx=3, freq=P, phase=P, L=4, lo=0, hi=3, dx=P, lddx=3, stream=None)
    common = (dict(n=-1), dict(n=1 << 28), dict(C=0, ldx=0, hi=0), dict(C=4097, ldx=4097), dict(L=0), dict(L=33), dict(lo=-1), dict(lo=2, hi=1),
              dict(hi=4), dict(ldx=2), dict(ldy=26), dict(x=None), dict(freq=None), dict(phase=None))
    for fn, ok, tag, own in ((L.mink_posenc_fwd, fwd, b"posenc_fwd", (dict(y=None),)),
                             (L.mink_posenc_bwd, bwd, b"posenc_bwd", (dict(dy=None), dict(dx=None), dict(lddx=2)))):
        for bad in common + own:
            a = dict(ok, **bad)
            assert fn(*[a[k] for k in ok]) == -1, (tag, bad)
            assert tag in L.mink_last_error(), (tag, bad, L.mink_last_error())
        a = dict(ok, n=0, **{k: None for k in ok if ok[k] == P})
        assert fn(*[a[k] for k in ok]) == 0  # nothing to do, no launch, no pointer looked at


def test_trainer_and_eval_refuse_an_instance_head():
    from nerf_downstream_amd.co3d_3d.src.models import get_model
    from nerf_downstream_amd.co3d_3d.src.modules.segmentation_training import SegmentationTraining, refuse_instance_head

    torch.manual_seed(0)
    ins = get_model("Res16UNet14AIns", 3, 5)
    with pytest.raises(ValueError, match="no loss for the offsets"):
        SegmentationTraining(ins)
    with pytest.raises(ValueError, match="co3d_3d.eval"):
        refuse_instance_head(ins, "co3d_3d.eval")
    SegmentationTraining(get_model("Res16UNet14A", 3, 5))
    import inspect

    from nerf_downstream_amd.co3d_3d import eval as E

    assert "refuse_instance_head(model" in inspect.getsource(E.evaluate)
