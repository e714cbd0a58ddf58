"""CPU: multi-head attention away from the kernel -- the float64 restatement (tests/attn_restate.py) against an independent
per-(b, h, i) loop, its derived bounds against a float32 run (inside) and two deliberately wrong variants (outside), the
argument checks of mink_attn_fwd / mink_attn_bwd (refused before any launch), the model surface of the 2-D Vision Transformers
(routing, timm's state-dict layout, parameter counts) and their gin files."""
import math
import os

import pytest
import torch

import attn_restate as AR
from nerf_downstream_amd import gin_lite as gin

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, "nerf_downstream_amd", "co3d_2d", "configs")
NAMES = {"vit_small_patch16_224": (384, 12, 6), "vit_base_patch16_224": (768, 12, 12), "vit_large_patch16_224": (1024, 24, 16)}


@pytest.fixture(autouse=True)
def _clean_gin():
    gin.clear_config()
    yield
    gin.clear_config()


def test_restatement_matches_an_independent_loop():
    B, H, N = 2, 2, 5
    q, k, v, dout = (t.double() for t in AR.inputs(B, H, N, seed=3))
    scale = 0.125
    f = AR.forward(q, k, v, scale)
    dq, dk, dv = AR.gradients(q, k, v, scale, dout)
    edq, edk, edv = torch.zeros_like(q), torch.zeros_like(k), torch.zeros_like(v)
    for b in range(B):
        for h in range(H):
            for i in range(N):
                s = [scale * sum(float(q[b, h, i, d]) * float(k[b, h, j, d]) for d in range(64)) for j in range(N)]
                m = max(s)
                e = [math.exp(x - m) for x in s]
                w = [x / sum(e) for x in e]
                assert abs(f["lse"][b, h, i] - (m + math.log(sum(e)))) < 1e-12 and abs(f["m"][b, h, i] - m) < 1e-12
                o = [sum(w[j] * float(v[b, h, j, d]) for j in range(N)) for d in range(64)]
                assert max(abs(float(f["o"][b, h, i, d]) - o[d]) for d in range(64)) < 1e-12
                assert max(abs(float(f["w"][b, h, i, j]) - w[j]) for j in range(N)) < 1e-14
                # the backward of the module docstring, row i's share
                delta = sum(float(dout[b, h, i, d]) * o[d] for d in range(64))
                for j in range(N):
                    dp = sum(float(dout[b, h, i, d]) * float(v[b, h, j, d]) for d in range(64))
                    ds = w[j] * (dp - delta)
                    edv[b, h, j] += w[j] * dout[b, h, i]
                    edq[b, h, i] += scale * ds * k[b, h, j]
                    edk[b, h, j] += scale * ds * q[b, h, i]
    for got, want in ((dq, edq), (dk, edk), (dv, edv)):
        assert (got - want).abs().max() < 1e-12
    # the row helpers are inverses of each other and follow the packed layout: column s H D + h D + d
    rows = AR.pack_rows(q, k, v)
    assert rows.shape == (B * N, 3 * H * 64) and rows[1 * N + 3, 2 * H * 64 + 1 * 64 + 7] == v[1, 1, 3, 7]
    for a, b_ in zip(AR.split_rows(rows, B, N, H), (q, k, v)):
        assert torch.equal(a, b_)
    assert torch.equal(AR.heads_of(AR.rows_of(q), B, N, H), q)


@pytest.mark.parametrize("kind", ["normal", "wide", "offset"])
def test_bounds_hold_for_a_float32_run_and_refuse_wrong_variants(kind):
    B, H, N = 1, 2, 37
    q, k, v, dout = AR.inputs(B, H, N, seed=11, kind=kind)
    scale = 0.125
    ref = AR.forward(q, k, v, scale)
    rdq, rdk, rdv = AR.gradients(q, k, v, scale, dout)
    bd = AR.bounds(q, k, v, scale, dout)
    if kind == "wide":
        assert ref["s"].abs().max() > 199
    f32 = AR.forward(q, k, v, scale, dtype=torch.float32)
    g32 = AR.gradients(q, k, v, scale, dout, dtype=torch.float32)
    ratios = {"o": AR.worst(f32["o"], ref["o"], bd["o"]), "lse": AR.worst(f32["lse"], ref["lse"], bd["lse"]),
              "dq": AR.worst(g32[0], rdq, bd["dq"]), "dk": AR.worst(g32[1], rdk, bd["dk"]), "dv": AR.worst(g32[2], rdv, bd["dv"])}
    print(kind, {n: f"{r:.3f}" for n, r in ratios.items()})
    assert all(r <= 1 for r in ratios.values()), ratios
    # twice the scale: far outside every bound
    bad = AR.forward(q, k, v, scale, dtype=torch.float32, variant="scale_twice")
    assert AR.worst(bad["o"], ref["o"], bd["o"]) > 1 and AR.worst(bad["lse"], ref["lse"], bd["lse"]) > 1
    bdq, bdk, bdv = AR.gradients(q, k, v, scale, dout, dtype=torch.float32, variant="scale_twice")
    assert AR.worst(bdq, rdq, bd["dq"]) > 1 and AR.worst(bdk, rdk, bd["dk"]) > 1 and AR.worst(bdv, rdv, bd["dv"]) > 1
    if kind == "wide":  # exp(200) is not an fp32 number: without the maximum the result is inf / NaN
        bad = AR.forward(q, k, v, scale, dtype=torch.float32, variant="no_max")
        assert AR.worst(bad["o"], ref["o"], bd["o"]) == math.inf


def test_attention_arguments_are_refused_before_any_launch():
    from nerf_downstream_amd import _lib

    L = _lib.lib()
    C = _lib.CONSTANTS
    assert C["MINK_ABI_VERSION"] == 4 and L.mink_abi_version() == 4
    assert C["MINK_ATTN_HEAD_DIM"] == 64 and C["MINK_ATTN_MAX_TOKENS"] >= 1024
    P = 0x10000  # aligned, never dereferenced: every call below is refused before a launch
    B, N, H, D = 2, 17, 3, 64
    need = L.mink_attn_bwd_workspace_bytes(B, N, H, D)
    assert need >= B * N * H * 4
    ok = dict(qkv=P, ldq=3 * H * D, out=P, ldo=H * D, lse=P, dout=P, lddo=H * D, B=B, N=N, H=H, D=D, dqkv=P, lddq=3 * H * D, ws=P,
              ws_bytes=need)

    def fwd(**kw):
        a = dict(ok, **kw)
        return L.mink_attn_fwd(a["qkv"], a["ldq"], a["B"], a["N"], a["H"], a["D"], 0.125, a["out"], a["ldo"], a["lse"], None)

    def bwd(**kw):
        a = dict(ok, **kw)
        return L.mink_attn_bwd(a["qkv"], a["ldq"], a["out"], a["ldo"], a["lse"], a["dout"], a["lddo"], a["B"], a["N"], a["H"], a["D"],
                               0.125, a["dqkv"], a["lddq"], a["ws"], a["ws_bytes"], None)

    big = C["MINK_ATTN_MAX_TOKENS"] + 1
    shared = [({"D": 32}, b"D=32"), ({"D": 128}, b"D=128"), ({"N": 0}, b"N=0"), ({"N": big}, b"N=%d" % big), ({"H": 0}, b"H=0"),
              ({"B": 0}, b"B=0"), ({"ldq": 3 * H * D - 1}, b"ldq=575"), ({"ldo": H * D - 1}, b"ldo=191"),
              ({"qkv": None}, b"NULL pointer (qkv"), ({"out": None}, b"NULL pointer"), ({"lse": None}, b"NULL pointer"),
              ({"qkv": P + 2}, b"4-byte aligned")]
    for call, cases in ((fwd, shared), (bwd, shared + [
            ({"dout": None}, b"NULL pointer"), ({"dqkv": None}, b"NULL pointer"), ({"ws": None}, b"NULL pointer"),
            ({"lddo": H * D - 1}, b"lddo=191"), ({"lddq": 3 * H * D - 1}, b"lddq=575"),
            ({"ws_bytes": need - 1}, b"workspace of %d bytes" % (need - 1)), ({"ws_bytes": 0}, b"workspace of 0 bytes"),
            ({"ws": P + 4}, b"workspace of")])):
        for kw, word in cases:
            assert call(**kw) == -1, kw
            assert word in L.mink_last_error(), (kw, L.mink_last_error())
    assert L.mink_attn_bwd_workspace_bytes(0, N, H, D) == 0


def test_select_model_routes_the_vit_names():
    from nerf_downstream_amd.co3d_2d.src.model.models import ResNetBased, ViTBased, select_model

    for name in NAMES:
        gin.bind_parameter("ViTBased.img_size", 32)  # (the routing passes the name alone; the size is a binding)
        assert type(select_model(name)) is ViTBased
    assert type(select_model("resnet18")) is ResNetBased
    for name in ("deit3_small_patch16_224", "nope"):
        with pytest.raises(NameError, match="Unknown model name"):
            select_model(name)
    with pytest.raises(NameError):
        select_model(None)


def expected_state(dim, depth, tokens):
    want = {"cls_token": (1, 1, dim), "pos_embed": (1, tokens, dim), "patch_embed.proj.weight": (dim, 3, 16, 16),
            "patch_embed.proj.bias": (dim,), "norm.weight": (dim,), "norm.bias": (dim,), "head.weight": (51, dim), "head.bias": (51,)}
    for i in range(depth):
        p = f"blocks.{i}."
        want.update({p + "norm1.weight": (dim,), p + "norm1.bias": (dim,), p + "attn.qkv.weight": (3 * dim, dim),
                     p + "attn.qkv.bias": (3 * dim,), p + "attn.proj.weight": (dim, dim), p + "attn.proj.bias": (dim,),
                     p + "norm2.weight": (dim,), p + "norm2.bias": (dim,), p + "mlp.fc1.weight": (4 * dim, dim),
                     p + "mlp.fc1.bias": (4 * dim,), p + "mlp.fc2.weight": (dim, 4 * dim), p + "mlp.fc2.bias": (dim,)})
    return {"model." + k: v for k, v in want.items()}


def parameter_count(dim, depth, tokens=197):
    block = 2 * 2 * dim + (3 * dim * dim + 3 * dim) + (dim * dim + dim) + (4 * dim * dim + 4 * dim) + (4 * dim * dim + dim)
    return (dim * 768 + dim) + dim + tokens * dim + depth * block + 2 * dim + (51 * dim + 51)


def test_vit_state_dict_is_timms_layout():
    from nerf_downstream_amd.co3d_2d.src.model.models import ViTBased

    assert parameter_count(384, 12) == 21_685_299  # 295,296 patch + 384 + 75,648 + 12 x 1,774,464 + 768 + 19,635 head
    for name, (dim, depth, heads) in NAMES.items():
        if name == "vit_large_patch16_224":  # 303 M parameters: its layout is the same code with other numbers
            continue
        net = ViTBased(name)
        sd = net.state_dict()
        assert {k: tuple(v.shape) for k, v in sd.items()} == expected_state(dim, depth, 197)
        assert sum(p.numel() for p in net.parameters()) == parameter_count(dim, depth), name
        assert all(blk.attn.num_heads == heads for blk in net.model.blocks)
    large = ViTBased("vit_large_patch16_224", img_size=32)
    assert {k: tuple(v.shape) for k, v in large.state_dict().items()} == expected_state(1024, 24, 5)
    assert sum(p.numel() for p in large.parameters()) == parameter_count(1024, 24, 5)
    # the initialisation the module states: biases 0, LayerNorm 1 / 0, linear weights inside the truncation of std 0.02
    small = ViTBased("vit_small_patch16_224", img_size=32)
    sd = small.state_dict()
    assert tuple(sd["model.pos_embed"].shape) == (1, 5, 384)
    assert float(sd["model.blocks.3.attn.qkv.bias"].abs().max()) == 0 and float(sd["model.head.bias"].abs().max()) == 0
    assert torch.equal(sd["model.blocks.0.norm1.weight"], torch.ones(384)) and float(sd["model.norm.bias"].abs().max()) == 0
    w = sd["model.blocks.5.mlp.fc1.weight"]
    assert 0.015 < float(w.std()) < 0.025 and float(w.abs().max()) <= 2.0
    with pytest.raises(ValueError, match="multiple of the patch size"):
        ViTBased("vit_small_patch16_224", img_size=40)
    with pytest.raises(NotImplementedError, match="pretrained"):
        ViTBased("vit_small_patch16_224", pretrained=True)
    with pytest.raises(NameError):
        ViTBased("resnet18")
    # a checkpoint in timm's layout loads, strictly
    other = ViTBased("vit_small_patch16_224", img_size=32)
    other.load_state_dict({k: v.clone() for k, v in sd.items()}, strict=True)
    assert all(torch.equal(a, b) for a, b in zip(other.state_dict().values(), sd.values()))


@pytest.mark.parametrize("tag,name", [("vitsmall", "vit_small_patch16_224"), ("vitbase", "vit_base_patch16_224"),
                                      ("vitlarge", "vit_large_patch16_224")])
def test_vit_configs_parse(tag, name):
    gin.parse_config_files_and_bindings([os.path.join(CFG, tag + ".gin")], [])
    assert gin.query_parameter("LitModel.model_name") == name
    assert gin.query_parameter("run.run_name") == f"co3d_perfception_{tag}_scratch"
    assert gin.query_parameter("run.precision") == 32
    assert gin.query_parameter("DataModule.train_co3d") is False and gin.query_parameter("DataModule.eval_co3d") is False
    ref = {}
    gin.clear_config()
    gin.parse_config_file(os.path.join(CFG, "resnet18.gin"))
    for key in ("DataModule.batch_size", "DataModule.num_workers"):
        ref[key] = gin.query_parameter(key)
    gin.clear_config()
    gin.parse_config_file(os.path.join(CFG, tag + ".gin"))
    assert all(gin.query_parameter(k) == v for k, v in ref.items())
