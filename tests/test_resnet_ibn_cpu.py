"""CPU: the ResNet-IBN baseline's module shells (state_dict, seeded initialisation, checkpoint loading) and the host-side weight
pack + BatchNorm fold (ops.pack_conv_bn) against a direct fp64 evaluation. Fixtures: tests/golden/make_resnet_golden.py."""
import json
import os

import pytest
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def lib():
    from neuralsampleid_amd.build import build_lib
    return build_lib(verbose=False)


@pytest.fixture(scope="module")
def keys():
    with open(os.path.join(GOLDEN, "resnet_ibn_keys.json")) as f:
        return json.load(f)


def _model(seed=None):
    from neuralsampleid_amd.encoder.resnet_ibn import ResNetIBN
    from neuralsampleid_amd.simclr.triplet import BaselineModel
    if seed is not None:
        torch.manual_seed(seed)
    return BaselineModel({}, ResNetIBN())


def test_state_dict_keys_shapes_and_seeded_init(lib, keys):
    model = _model(keys["init_seed"])
    sd = model.state_dict()
    assert len(sd) == 193 == len(keys["keys"])
    assert [[k, list(v.shape)] for k, v in sd.items()] == keys["keys"]
    assert sum(p.numel() for p in model.parameters()) == keys["params"]
    for k, v in sd.items():                       # same construction order: the seeded default initialisation draws the same values
        s, n = keys["init"][k]
        assert abs(float(v.double().sum()) - s) <= 1e-9 * max(1.0, abs(s)) + 1e-12, k
        assert abs(float(v.double().norm()) - n) <= 1e-9 * max(1.0, n), k
    assert isinstance(model.projector, torch.nn.Identity)


@pytest.mark.parametrize("prefix", ["", "module."])
def test_reference_checkpoint_loads_strictly(lib, prefix):
    from synth import synth_state
    from neuralsampleid_amd.checkpoint import is_baseline_state, simclr_for_checkpoint
    from neuralsampleid_amd.encoder.resnet_ibn import ResNetIBN
    from neuralsampleid_amd.simclr.triplet import BaselineModel
    src = synth_state(_model().state_dict())
    ckpt = {"epoch": 3, "loss": [1.0], "hit_rate_log": [], "optimizer": None, "scheduler": None,
            "state_dict": {prefix + k: v for k, v in src.items()}}
    assert is_baseline_state(ckpt["state_dict"])
    model = simclr_for_checkpoint({"arch": "resnet-ibn", "n_frames": 216}, ckpt)
    assert isinstance(model, BaselineModel) and isinstance(model.encoder, ResNetIBN)
    got = model.state_dict()
    assert list(got) == list(src) and all(torch.equal(got[k], src[k]) for k in src)
    broken = dict(ckpt["state_dict"])
    broken.pop(prefix + "encoder.layer3.0.downsample.1.running_var")
    with pytest.raises(RuntimeError):             # strict
        simclr_for_checkpoint({}, {"state_dict": broken})


def test_graph_encoder_checkpoints_are_not_taken_for_the_baseline(lib):
    from synth import GRAFP_CFG, synth_state
    from neuralsampleid_amd.checkpoint import is_baseline_state, simclr_for_checkpoint
    from neuralsampleid_amd.encoder.graph_encoder import GraphEncoder
    from neuralsampleid_amd.simclr.simclr import SimCLR
    sd = synth_state(SimCLR(GRAFP_CFG, GraphEncoder(GRAFP_CFG, in_channels=8, k=3, size="t")).state_dict())
    assert not is_baseline_state(sd)
    assert isinstance(simclr_for_checkpoint(GRAFP_CFG, {"state_dict": sd}, size="t"), SimCLR)


@pytest.mark.parametrize("shape", [(128, 64, 3), (256, 128, 1), (64, 1, 7), (8, 16, 3)], ids=lambda s: "Co%dC%dk%d" % s)
def test_pack_and_fold_against_fp64(lib, shape):
    """conv(x; pack) + bias == BN(conv(x; w)) elementwise, with the packed matrix applied to explicitly gathered taps (kh, kw, c)"""
    from neuralsampleid_amd import ops
    Co, C, k = shape
    g = torch.Generator().manual_seed(11 * Co + C + k)
    w = torch.randn(Co, C, k, k, generator=g) * (C * k * k) ** -0.5
    gamma, beta = 1.0 + 0.1 * torch.randn(Co, generator=g), 0.1 * torch.randn(Co, generator=g)
    mean, var = 0.1 * torch.randn(Co, generator=g), 0.5 + torch.rand(Co, generator=g)
    wp, bias = ops.pack_conv_bn(w, gamma, beta, mean, var, 1e-5)
    assert wp.shape == (Co, k * k * C) and wp.is_contiguous() and bias.shape == (Co,)
    x = torch.randn(2, C, 9, 8, generator=g).double() + 0.5
    F = torch.nn.functional
    ref = F.batch_norm(F.conv2d(x, w.double(), padding=k // 2), mean.double(), var.double(), gamma.double(), beta.double(), False, 0.0, 1e-5)
    xp = F.pad(x, (k // 2,) * 4)
    taps = torch.stack([xp[:, :, kh:kh + 9, kw:kw + 8] for kh in range(k) for kw in range(k)], 1)     # (B, taps, C, H, W)
    got = torch.einsum("btchw,otc->bohw", taps, wp.double().view(Co, k * k, C)) + bias.double().view(1, -1, 1, 1)
    assert float((got - ref).norm() / ref.norm()) < 2e-7          # fp32 rounding of the folded weights, nothing else
    raw, none = ops.pack_conv_bn(w)
    assert none is None and torch.equal(raw.view(Co, k, k, C).permute(0, 3, 1, 2), w)


def test_training_mode_and_cpu_tensors_raise(lib):
    model = _model()
    with pytest.raises(NotImplementedError, match="eval"):
        model.train()(torch.zeros(1, 84, 216), torch.zeros(1, 84, 216))
    with pytest.raises(NotImplementedError, match="CPU"):
        model.eval()(torch.zeros(1, 84, 216), torch.zeros(1, 84, 216))


def test_consumer_shapes_come_from_the_model(lib):
    from neuralsampleid_amd.fingerprint import embedding_dim, input_shape
    model = _model()
    assert embedding_dim(model) == 2048
    assert input_shape(model) == (84, 216)
    model.cfg = {"n_frames": 100, "n_mels": 64}
    assert input_shape(model) == (84, 100)
