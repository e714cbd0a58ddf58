"""-m gpu: EncodedRes16UNet, EncodedRes16UNet2 and Res16UNet14AIns, one training-mode step on two 32^3 shell scenes, against the
same network in float64 on the CPU oracle's maps; and the trainer CLI on the encoded network.

The oracle namespace (oracle/me_cpu.py) holds neither per-point layers nor the encoding; `_OracleME` supplies them the way
tests/test_gpu_norm.py::_OracleME supplies the layer norm: MinkowskiLinear and a ReLU that keep a field a field, ME.cat of fields,
`TensorField.sparse(quantization_mode=)` as the oracle's autograd-aware mean, and the encoding as the float64 restatement of
tests/posenc_restate.py on the layer's own constants.

Tolerances: those of tests/test_gpu_unet.py::test_res16unet_matches_oracle -- logits within 1e-3; per-tensor relative gradient
error below 0.15, its median below 2e-2, cosine of the flattened gradients above 0.999."""
import enum
import os
import re
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

import posenc_restate as R
from helpers import batch_scenes

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, "nerf_downstream_amd", "co3d_3d", "configs")


class _OracleME:
    def __init__(self):
        from oracle import me_cpu as OME

        self._ome = OME

        class TensorField(OME.TensorField):
            def sparse(self, quantization_mode=None):
                assert quantization_mode is None or quantization_mode.name == "UNWEIGHTED_AVERAGE"
                return super().sparse()

        def same_kind(input, feats):
            if isinstance(input, OME.TensorField):
                return TensorField(features=feats, coordinates=input.C, _manager=input._manager)
            return OME.SparseTensor(feats, input.coordinate_map_key, input._manager)

        class MinkowskiLinear(torch.nn.Module):
            def __init__(self, in_features, out_features, bias=True):
                super().__init__()
                self.linear = torch.nn.Linear(in_features, out_features, bias=bias)

            def forward(self, input):
                return same_kind(input, self.linear(input.F))

        class MinkowskiReLU(torch.nn.Module):
            def __init__(self, inplace=False):
                super().__init__()

            def forward(self, input):
                return same_kind(input, torch.relu(input.F))

        class MinkowskiPositionalEncoding(torch.nn.Module):
            """The restatement on this layer's constants (the HIP layer's fp32 values, widened when the network is)."""

            def __init__(self, in_channel, num_encoding_functions=4):
                super().__init__()
                chan, freq, phase = R.columns(in_channel, num_encoding_functions)
                P = lambda t: torch.nn.Parameter(t, requires_grad=False)  # noqa: E731
                self.coo = P(torch.stack([chan, torch.arange(chan.numel())]))
                self.frequencies, self.offset = P(freq.float()), P(phase.float().view(1, -1))
                self.out_channels = chan.numel()

            def forward(self, input):
                y = R.forward(input.F, self.coo[0], self.frequencies, self.offset.view(-1))
                return same_kind(input, y.to(self.frequencies.dtype))

        def cat(*tensors):
            if isinstance(tensors[0], OME.TensorField):
                assert all(t._manager is tensors[0]._manager for t in tensors)
                return same_kind(tensors[0], torch.cat([t.F for t in tensors], dim=1))
            return OME.cat(*tensors)

        class SparseTensorQuantizationMode(enum.Enum):
            UNWEIGHTED_AVERAGE = 1

        self.TensorField, self.MinkowskiLinear, self.MinkowskiReLU, self.cat = TensorField, MinkowskiLinear, MinkowskiReLU, cat
        self.MinkowskiPositionalEncoding, self.SparseTensorQuantizationMode = MinkowskiPositionalEncoding, SparseTensorQuantizationMode

    def __getattr__(self, name):
        return getattr(self._ome, name)


def _scenes(cin):
    """Two 32^3 shell scenes as a float field: jittered inside their voxels, a fifth of the points doubled (with other features),
    so that `.sparse()` averages and `slice` fans out."""
    coords, feats = batch_scenes([71, 72], grid=32, cin=cin)
    rng = torch.Generator().manual_seed(3)
    coords = coords.clone()
    coords[:, 1:] += torch.rand(coords.shape[0], 3, generator=rng) * 0.9
    extra = torch.randint(0, coords.shape[0], (coords.shape[0] // 5,), generator=rng).sort().values
    dup = coords[extra].clone()
    dup[:, 1:] = dup[:, 1:].floor() + torch.rand(extra.numel(), 3, generator=rng) * 0.9
    order = torch.argsort(torch.cat([coords[:, 0], dup[:, 0]]), stable=True)
    return torch.cat([coords, dup])[order], torch.cat([feats, feats[extra] * 0.5 + 0.3])[order]


def _compare_gradients(hip, ref, what, zero_by_construction=()):
    """`zero_by_construction`: parameters whose exact gradient is zero, so that a relative error is 0 / 0 (float64 leaves
    1e-17 of rounding there); the caller holds them to an absolute bound of their own, every other tensor is compared here."""
    hp = {k: p for k, p in hip.named_parameters() if p.requires_grad}
    rp = {k: p for k, p in ref.named_parameters() if p.requires_grad}
    assert hp.keys() == rp.keys()
    assert all(p.grad is not None for p in hp.values()), [k for k, p in hp.items() if p.grad is None]
    frozen = {k: p for k, p in hip.named_parameters() if not p.requires_grad}
    assert all(p.grad is None for p in frozen.values())
    assert all(k in hp for k in zero_by_construction)
    hp = {k: p for k, p in hp.items() if k not in zero_by_construction}
    rel = {k: float((hp[k].grad.cpu().double() - rp[k].grad).norm() / rp[k].grad.norm().clamp_min(1e-12)) for k in hp}
    flat_g = torch.cat([hp[k].grad.cpu().double().flatten() for k in hp])
    flat_o = torch.cat([rp[k].grad.flatten() for k in hp])
    cos = float(torch.dot(flat_g, flat_o) / (flat_g.norm() * flat_o.norm()))
    worst, errs = max(rel.items(), key=lambda kv: kv[1]), sorted(rel.values())
    print(f"[{what}] parameter gradients: worst {worst[0]} {worst[1]:.2e}, median {errs[len(errs) // 2]:.2e}, cosine {cos:.6f}")
    assert worst[1] < 0.15, worst
    assert errs[len(errs) // 2] < 2e-2, errs[len(errs) // 2]
    assert cos > 0.999, cos
    return frozen


def _pair(name, cin, ncls):
    from nerf_downstream_amd.co3d_3d.src.models import get_model

    torch.manual_seed(0)
    ref = get_model(name, cin, ncls, ME=_OracleME()).double()
    hip = get_model(name, cin, ncls).cuda()
    hip.load_state_dict({k: (v.float() if v.is_floating_point() else v) for k, v in ref.state_dict().items()})
    return hip.train(), ref.train()


@pytest.mark.parametrize("name", ["EncodedRes16UNet", "EncodedRes16UNet2"])
def test_encoded_unet_matches_float64(oracle_maps, name):
    cin, ncls = 3, 20
    hip, ref = _pair(name, cin, ncls)
    coords, feats = _scenes(cin)
    labels = torch.randint(0, ncls, (coords.shape[0],), generator=torch.Generator().manual_seed(4))
    field = hip.process_input({"coordinates": coords.cuda(), "features": feats.cuda()})
    out = hip(field)
    assert field.coordinate_manager.levels[1].n < coords.shape[0]  # duplicates: .sparse() averaged
    out64 = ref(ref.process_input({"coordinates": coords, "features": feats.double()}))
    assert out.shape == (coords.shape[0], ncls) == out64.shape
    err = float((out.detach().cpu().double() - out64).abs().max())
    print(f"[{name}] logits: max |err| {err:.2e} against float64 (max |logit| {float(out64.abs().max()):.2f})")
    assert err <= 1e-3
    F.cross_entropy(out, labels.cuda()).backward()
    F.cross_entropy(out64, labels).backward()
    frozen = _compare_gradients(hip, ref, name)
    assert sorted(frozen) == ["encoding.coo", "encoding.frequencies", "encoding.offset"]
    assert any(k.startswith("enc_mlp.0.0") for k, p in hip.named_parameters() if p.grad is not None)  # through .sparse() to the points


def test_instance_variant_matches_float64(oracle_maps):
    cin, ncls = 3, 20
    hip, ref = _pair("Res16UNet14AIns", cin, ncls)
    coords, feats = _scenes(cin)
    g = torch.Generator().manual_seed(5)
    labels = torch.randint(0, ncls, (coords.shape[0],), generator=g)
    target = torch.randn(coords.shape[0], 3, generator=g)
    seen = {}  # of the float64 run: z = the head's first convolution output, dz = its gradient, g = the gradient behind the norm

    def keep(value, gradient):
        def hook(module, inputs, output):  # (returns None: the output stays what it is)
            if value is not None:
                seen[value] = output.F.detach()
            output.F.register_hook(lambda t: seen.__setitem__(gradient, t.detach()))

        return hook

    ref.offset_block[0].register_forward_hook(keep("z", "dz"))
    ref.offset_block[1].register_forward_hook(keep(None, "g"))
    off, out = hip(hip.process_input({"coordinates": coords.cuda(), "features": feats.cuda()}))
    off64, out64 = ref(ref.process_input({"coordinates": coords, "features": feats.double()}))
    assert off.shape == (coords.shape[0], 3) == off64.shape and out.shape == (coords.shape[0], ncls) == out64.shape
    for what, a, b in (("offsets", off, off64), ("logits", out, out64)):
        err = float((a.detach().cpu().double() - b).abs().max())
        print(f"[Res16UNet14AIns] {what}: max |err| {err:.2e} against float64 (max |value| {float(b.abs().max()):.2f})")
        assert err <= 1e-3
    (F.cross_entropy(out, labels.cuda()) + F.mse_loss(off, target.cuda())).backward()
    (F.cross_entropy(out64, labels) + F.mse_loss(off64, target.double())).backward()
    assert not _compare_gradients(hip, ref, "Res16UNet14AIns", zero_by_construction=("offset_block.0.bias",))
    assert hip.offset_block[3].kernel.grad is not None and hip.final.kernel.grad is not None
    # offset_block.0.bias sits in front of a training-mode batch norm, which removes it: its gradient is the column sum of
    # dz = gamma invstd (g - mean g - xhat mean(g xhat)), exactly zero.  What fp32 leaves is rounding: each dz element is off by
    # a few roundings of its three terms T = |gamma| invstd (|g| + |mean g| + |xhat| |mean(g xhat)|) (8 u T covers them), and a
    # sum of n fp32 numbers in ANY order is off by at most (n - 1) u sum |dz|, u = 2^-24.  Both from the float64 run's tensors.
    bn = ref.offset_block[1].bn
    z, dz, g = seen["z"], seen["dz"], seen["g"]
    n, u = z.shape[0], 2.0 ** -24
    invstd = (z.var(0, unbiased=False) + bn.eps).rsqrt()
    xhat = (z - z.mean(0)) * invstd
    T = bn.weight.detach().abs() * invstd * (g.abs() + g.mean(0).abs() + xhat.abs() * (g * xhat).mean(0).abs())
    bound = u * (n * dz.abs().sum(0) + 8 * T.sum(0))
    g64, g32 = ref.offset_block[0].bias.grad.view(-1), hip.offset_block[0].bias.grad.cpu().double().view(-1)
    print(f"[Res16UNet14AIns] offset_block.0.bias (exact gradient 0): float64 max |g| {float(g64.abs().max()):.1e}, fp32 max |g| "
          f"{float(g32.abs().max()):.1e}, max |g| / bound {float((g32.abs() / bound).max()):.3f}, sum |dz| per channel up to {float(dz.abs().sum(0).max()):.2e}")
    assert float(g64.abs().max()) <= 1e-12 * float(dz.abs().sum(0).max())
    assert bool((g32.abs() <= bound).all())


@pytest.mark.long
@pytest.mark.timeout(170)
def test_trainer_cli_on_the_encoded_network(tmp_path):
    cmd = ["timeout", "-k", "10", "150", sys.executable, "-m", "nerf_downstream_amd.co3d_3d.train", "--ginc", f"{CFG}/co3d_cls.gin",
           "--ginc", f"{CFG}/synthetic_seg.gin", "--ginc", f"{CFG}/encoded_res16unet.gin", "--save_path", str(tmp_path), "--run_name", "enc",
           "--gpus", "1", "--seed", "2"]
    for b in ("train.max_steps=3", "train.val_every_n_steps=3", "train.log_every_n_steps=1", "train.batch_size=2", "train.val_batch_size=2",
              "SparseVoxelSegDataset.grid=32", "SparseVoxelSegDataset.num_samples=8", "train.lr=0.01"):
        cmd += ["--ginb", b]
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True)
    text = r.stdout + r.stderr
    assert r.returncode == 0, text[-4000:]
    losses = [float(v) for v in re.findall(r"step \d+: train/loss=(\S+)", text)]
    assert len(losses) == 3 and all(torch.isfinite(torch.tensor(losses))), text[-3000:]
    assert "EncodedRes16UNet" in text or (tmp_path / "enc").exists()
