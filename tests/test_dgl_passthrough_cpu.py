"""CPU: the module tree of the DGL-variant passthrough encoder against the reference's GraphEncoderDGL (tests/golden/dgl_keys.json,
made by tests/golden/make_dgl_golden.py), strict checkpoint round trips, the class-by-checkpoint helper and the refusals."""
import json
import os

import pytest
import torch

from synth import GRAFP_CFG, synth_state

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _enc(size="t", **kw):
    from neuralsampleid_amd.encoder.dgl.passthrough import PassthroughGraphEncoderDGL
    return PassthroughGraphEncoderDGL(cfg=GRAFP_CFG, in_channels=GRAFP_CFG["n_filters"], k=3, size=size, **kw)


def _simclr(enc):
    from neuralsampleid_amd.simclr.simclr import SimCLR
    m = SimCLR(GRAFP_CFG, enc)
    m.load_state_dict(synth_state(m.state_dict()))
    return m


@pytest.mark.parametrize("size", ["t", "s", "m", "b"])
def test_state_dict_names_and_shapes_match_reference(size):
    ref = json.load(open(os.path.join(GOLDEN, "dgl_keys.json")))[size]
    enc = _enc(size)
    assert [[k, list(v.shape)] for k, v in enc.state_dict().items()] == ref["keys"]
    assert sum(p.numel() for p in enc.parameters()) == ref["params"]


def test_live_part_of_size_t():
    """449 keys / 15.5 M parameters, of which the stem, the three Downsample layers and proj reach the output: 29 keys, 1.04 M"""
    enc = _enc("t")
    assert len(enc.state_dict()) == 449
    live = {pre + k: v for pre, m in enc.live_modules() for k, v in m.state_dict().items()}
    assert len(live) == 29
    n = sum(p.numel() for _, m in enc.live_modules() for p in m.parameters())
    assert 1.03e6 < n < 1.05e6, n
    assert [m.conv[0].weight.shape for m in enc.downsamples()] == [(128, 64, 3), (256, 128, 3), (512, 256, 3)]


@pytest.mark.parametrize("prefix", ["", "module."])
def test_checkpoint_round_trip_strict(tmp_path, prefix):
    from neuralsampleid_amd.checkpoint import load_reference_checkpoint, save_reference_checkpoint
    src = _simclr(_enc("t"))
    path = str(tmp_path / "model.pth")
    save_reference_checkpoint(path, src, epoch=35)
    if prefix:       # what nn.DataParallel training writes (train.py:117-120)
        ck = torch.load(path, weights_only=True)
        ck["state_dict"] = {prefix + k: v for k, v in ck["state_dict"].items()}
        torch.save(ck, path)
    dst = _simclr(_enc("t"))
    with torch.no_grad():
        for t in dst.state_dict().values():
            if t.is_floating_point():
                t.zero_()
    ck = load_reference_checkpoint(dst, path)
    assert ck["epoch"] == 35
    a, b = src.state_dict(), dst.state_dict()
    assert list(a) == list(b) and all(torch.equal(a[k], b[k]) for k in a)
    # the gcn_lib tree does not take it
    from neuralsampleid_amd.encoder.graph_encoder import GraphEncoder
    from neuralsampleid_amd.simclr.simclr import SimCLR
    with pytest.raises(RuntimeError):
        load_reference_checkpoint(SimCLR(GRAFP_CFG, GraphEncoder(GRAFP_CFG, in_channels=8, k=3, size="t")), path)


@pytest.mark.parametrize("prefix", ["", "module."])
def test_helper_chooses_encoder_class(prefix):
    from neuralsampleid_amd.checkpoint import encoder_variant, simclr_for_checkpoint
    from neuralsampleid_amd.encoder.dgl.passthrough import PassthroughGraphEncoderDGL
    from neuralsampleid_amd.encoder.graph_encoder import GraphEncoder
    from neuralsampleid_amd.simclr.simclr import SimCLR
    for size in ("t", "s"):
        dgl = _simclr(_enc(size))
        sd = {prefix + k: v for k, v in dgl.state_dict().items()}
        assert encoder_variant(sd) == "dgl"
        m = simclr_for_checkpoint(GRAFP_CFG, {"state_dict": sd, "epoch": 3})
        assert type(m.encoder) is PassthroughGraphEncoderDGL and m.encoder.channels == dgl.encoder.channels
        assert all(torch.equal(v, m.state_dict()[k]) for k, v in dgl.state_dict().items())
    gcn = SimCLR(GRAFP_CFG, GraphEncoder(GRAFP_CFG, in_channels=8, k=3, size="t"))
    sd = {prefix + k: v for k, v in gcn.state_dict().items()}
    assert encoder_variant(sd) == "gcn_lib"
    m = simclr_for_checkpoint(GRAFP_CFG, sd)
    assert type(m.encoder) is GraphEncoder
    with pytest.raises(KeyError):
        encoder_variant({"projector.0.weight": torch.zeros(2, 2)})


def test_refusals(monkeypatch):
    from neuralsampleid_amd.encoder.dgl import passthrough
    built = []
    monkeypatch.setattr(torch.nn.Module, "__init__", lambda self, *a, **k: built.append(self))
    with pytest.raises(NotImplementedError, match="conv='mr'"):
        passthrough.PassthroughGraphEncoderDGL(cfg=GRAFP_CFG, conv="edge")
    assert built == []                       # refused before anything is allocated
    monkeypatch.undo()
    with pytest.raises(NotImplementedError):
        _enc(act="swish")
    with pytest.raises(NotImplementedError):
        _enc(norm="layer")
    enc = _enc(norm=None)                    # the reference's norm=None: the graph blocks lose their BatchNorm, nothing else
    assert not any(".0.norm." in k for k in enc.state_dict())
