"""GPU: the DGL-variant passthrough encoder (encoder/dgl/passthrough.py, csrc/dsact.hip).

Kernels against a torch fp64 restatement; the whole model against the reference's own GraphEncoderDGL (tests/golden/
make_dgl_golden.py); the pipeline consumers; training semantics of the unused blocks; reproducibility."""
import hashlib
import json

import numpy as np
import pytest
import torch

from compare import SampledRef, maxerr, relerr

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ACTS = {"none": 0, "relu": 1, "leaky": 2}
SLOPE = {"none": 1.0, "relu": 0.0, "leaky": 0.2}
LIVE = ("peak_extractor.", "encoder.stem.", "encoder.backbone.2.", "encoder.backbone.5.", "encoder.backbone.12.", "encoder.proj.",
        "projector.")
# conv biases in front of a training-mode BatchNorm: analytically zero gradient, left at exactly 0 (functional.EXACT_BIAS_GRAD); the
# reference's value is its roundoff
BIAS_BEFORE_BN = ("encoder.backbone.2.conv.0.bias", "encoder.backbone.5.conv.0.bias", "encoder.backbone.12.conv.0.bias")


def _act64(v, act):
    return torch.where(v > 0, v, v * SLOPE[act]) if act != "none" else v


def _operands(B, N, C, Co, dt, seed):
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(B * N, C, generator=g) * 1.5).to(dt)
    w = torch.randn(Co, C, 3, generator=g) * (3 * C) ** -0.5
    bias = 0.1 * torch.randn(Co, generator=g)
    sc = 0.5 + torch.rand(C, generator=g)
    sh = 0.2 + 0.3 * torch.rand(C, generator=g)          # shift > 0: a prologue applied to the padding would show
    dr = torch.randn(B * ((N - 1) // 2 + 1), Co, generator=g).to(dt)
    mean, invstd = 0.1 * torch.randn(C, generator=g), 0.5 + torch.rand(C, generator=g)
    return x, w, bias, sc, sh, dr, mean, invstd


# (B, N, C, C'): B = 1 and odd B; N = 256 / 128 / 64; the size-'t' stages and size 's''s first one
SHAPES = [(1, 256, 64, 128), (3, 256, 64, 128), (5, 128, 128, 256), (2, 64, 256, 512), (3, 256, 80, 160), (7, 64, 128, 256)]


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("act", list(ACTS))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "B%dN%dC%dCo%d" % s)
def test_dsact_kernels_vs_fp64(shape, act, dt):
    from neuralsampleid_amd import ops
    B, N, C, Co = shape
    x, w, bias, sc, sh, dr, mean, invstd = _operands(B, N, C, Co, dt, 17 * B + N + C + ACTS[act])
    xc, wc, bc, drc = x.to(DEV), w.to(DEV), bias.to(DEV), dr.to(DEV)
    aff = ops.BNAffine(sc.to(DEV), sh.to(DEV), mean.to(DEV), invstd.to(DEV))
    tol = 2e-6 if dt == torch.float32 else 1e-2      # bf16: the output's storage rounding (2^-9 relative)

    # fp64 restatement: Conv1d(k3, s2, p1) of act(sc * x + sh) — the conv pads the ACTIVATED tensor
    pre = (x.double().reshape(B, N, C) * sc.double() + sh.double()).requires_grad_(True)
    wv = w.double().requires_grad_(True)
    y64 = torch.nn.functional.conv1d(_act64(pre, act).permute(0, 2, 1), wv, bias.double(), stride=2, padding=1)
    dpre, dw64 = torch.autograd.grad(y64, (pre, wv), dr.double().reshape(B, -1, Co).permute(0, 2, 1))
    ref = y64.detach().permute(0, 2, 1).reshape(-1, Co)

    # forward: output and BatchNorm partial statistics
    y, stat = ops.dsact_fwd(xc, B, N, C, wc, bc, Co, aff, ACTS[act], want_stat=True)
    assert y.dtype == dt and y.shape == ref.shape
    assert relerr(y.float().cpu(), ref) < tol, relerr(y.float().cpu(), ref)
    ys = y.double().cpu()
    assert stat.shape == (2, ops.row_tiles(ref.shape[0]), Co)
    assert relerr(stat[0].sum(0).cpu(), ys.sum(0)) < 1e-5
    assert relerr(stat[1].sum(0).cpu(), (ys * ys).sum(0)) < 1e-5

    # eval epilogue: this layer's BatchNorm affine + ReLU
    osc, osh = 0.5 + torch.rand(Co), 0.1 * torch.randn(Co)
    ye, none = ops.dsact_fwd(xc, B, N, C, wc, bc, Co, aff, ACTS[act], out_aff=ops.BNAffine(osc.to(DEV), osh.to(DEV)), act_out=1)
    assert none is None
    assert relerr(ye.float().cpu(), torch.relu(ref * osc.double() + osh.double())) < tol

    # weight gradient through the same prologue (accumulates)
    dw = torch.full((Co, C, 3), 0.25, device=DEV)
    ops.dsact_bwd_weight(drc, xc, dw, B, N, C, Co, aff, ACTS[act])
    assert relerr(dw.cpu() - 0.25, dw64) < 1e-5, relerr(dw.cpu() - 0.25, dw64)

    # data gradient: times the activation derivative of the layer in front, plus its BatchNorm-backward column sums
    g, part = ops.dsact_bwd_data(drc, wc, B, N, C, Co, xc, aff, ACTS[act], want_partial=True)
    g_ref = dpre.reshape(B * N, C)
    assert g.dtype == dt and g.shape == g_ref.shape
    assert relerr(g.float().cpu(), g_ref) < tol, relerr(g.float().cpu(), g_ref)
    assert part.shape[0] == 2 and part.shape[2] == C
    gs = g.double().cpu()
    xh = (x.double() - mean.double()) * invstd.double()
    assert relerr(part[0].sum(0).cpu(), gs.sum(0)) < 1e-5
    assert relerr(part[1].sum(0).cpu(), (gs * xh).sum(0)) < 1e-5


def _model(size="t", dt=torch.float32):
    from synth import GRAFP_CFG, synth_state
    from neuralsampleid_amd import functional as F_
    from neuralsampleid_amd.encoder.dgl.passthrough import PassthroughGraphEncoderDGL
    from neuralsampleid_amd.simclr.simclr import SimCLR
    F_.set_activation_dtype(dt)
    torch.manual_seed(1234)
    model = SimCLR(GRAFP_CFG, PassthroughGraphEncoderDGL(cfg=GRAFP_CFG, in_channels=GRAFP_CFG["n_filters"], k=3, size=size))
    model.load_state_dict(synth_state(model.state_dict()))
    return model.to(DEV)


@pytest.fixture
def restore():
    from neuralsampleid_amd import functional as F_
    defer = F_.DEFER_WGRAD
    yield
    F_.set_activation_dtype(torch.float32)
    F_.DEFER_WGRAD = defer
    F_.DIRECT_GRADS = False


def _clips(gold):
    from synth import synth_clips
    x_i, x_j = synth_clips(8)
    sha = hashlib.sha256(x_i.numpy().tobytes() + x_j.numpy().tobytes()).hexdigest()[:16]
    assert sha == bytes(gold["clips_sha"]).decode(), "synth_clips no longer reproduces the fixture's inputs"
    return x_i.to(DEV), x_j.to(DEV)


def _cos_rows(a, b):
    return torch.nn.functional.cosine_similarity(a.double().cpu(), torch.as_tensor(np.asarray(b)).double(), dim=1)


def _cos_ref(a, ref):
    a = a.detach().double().cpu().reshape(-1)
    if isinstance(ref, SampledRef):
        a, s = a[::ref.stride], torch.as_tensor(ref.sample)
    else:
        s = torch.as_tensor(np.asarray(ref)).double().reshape(-1)
    return float(torch.dot(a, s) / (a.norm() * s.norm()).clamp_min(1e-300))


def _step(model, x_i, x_j):
    from synth import GRAFP_CFG
    from neuralsampleid_amd.simclr.ntxent import ntxent_loss
    model.train()
    model.zero_grad(set_to_none=True)
    h_i, h_j, z_i, z_j = model(x_i, x_j)
    loss = ntxent_loss(z_i, z_j, GRAFP_CFG)
    loss.backward()
    torch.cuda.synchronize()
    return loss.detach(), z_i.detach(), z_j.detach()


def test_whole_model_fp32_vs_reference(golden, restore):
    gold = golden("dgl_passthrough_b8")
    model = _model()
    x_i, x_j = _clips(gold)
    model.eval()
    with torch.no_grad():
        h_i, _, z_i, z_j = model(x_i, x_j)
        nodes, emb = model.encoder(model.peak_extractor(x_i), return_pre_proj=True)
    assert nodes.shape == (8, 512, 32) and torch.equal(emb, h_i)
    assert maxerr(h_i.cpu(), gold.t("h_i_eval")) < 1e-5
    assert maxerr(z_i.cpu(), gold.t("z_i_eval")) < 1e-5 and maxerr(z_j.cpu(), gold.t("z_j_eval")) < 1e-5
    assert maxerr(nodes.cpu(), gold.t("nodes_i_eval")) < 1e-5

    loss, z_i, z_j = _step(model, x_i, x_j)
    assert abs(float(loss) - float(gold["loss_train"][0])) < 1e-5
    assert maxerr(z_i.cpu(), gold.t("z_i_train")) < 1e-5 and maxerr(z_j.cpu(), gold.t("z_j_train")) < 1e-5
    live = json.loads(bytes(gold["live_names"]).decode())
    errs = {}
    for n, p in model.named_parameters():
        if n not in live:
            assert p.grad is None, n
        elif n in BIAS_BEFORE_BN:
            assert float(p.grad.abs().max()) == 0.0 and maxerr(p.grad.cpu(), gold.t("grad." + n)) < 1e-5, n
        else:
            errs[n] = relerr(p.grad.cpu(), gold.t("grad." + n))
    assert len(errs) == 20 and max(errs.values()) < 1e-4, errs
    sd = model.state_dict()
    for k in [k for k in gold if k.startswith("bn.")]:
        got, want = sd[k[3:]].cpu(), gold.t(k)
        if k.endswith("num_batches_tracked"):
            assert int(got) == int(want) == 2, k
        else:
            assert relerr(got, want) < 1e-5, k


def test_whole_model_bf16_vs_reference(golden, restore):
    gold = golden("dgl_passthrough_b8")
    model = _model(dt=torch.bfloat16)
    x_i, x_j = _clips(gold)
    model.eval()
    with torch.no_grad():
        _, _, z_i, _ = model(x_i, x_j)
    ce = _cos_rows(z_i, gold["z_i_eval"]).min().item()
    _, z_i, _ = _step(model, x_i, x_j)
    ct = _cos_rows(z_i, gold["z_i_train"]).min().item()
    live = json.loads(bytes(gold["live_names"]).decode())
    cos = {n: _cos_ref(p.grad, gold.t("grad." + n)) for n, p in model.named_parameters() if n in live and n not in BIAS_BEFORE_BN}
    print(f"bf16: min row cos(z) eval {ce:.5f} train {ct:.5f}; min gradient cos {min(cos.values()):.5f}")
    assert ce >= 0.995 and ct >= 0.995, (ce, ct)
    assert min(cos.values()) >= 0.98, cos


@pytest.mark.parametrize("defer", [0, 1])
@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("opt_kind", ["adam", "fused"])
def test_unused_blocks_bitwise_unchanged(opt_kind, dt, defer, restore):
    from synth import GRAFP_CFG, synth_clips
    from neuralsampleid_amd import functional as F_
    from neuralsampleid_amd.optim import FusedClipAdam
    from neuralsampleid_amd.simclr.ntxent import ntxent_loss
    F_.DEFER_WGRAD = defer
    model = _model(dt=dt).train()
    before = {n: t.detach().clone() for n, t in model.state_dict().items()}
    params = dict(model.named_parameters())
    opt = torch.optim.Adam(model.parameters(), lr=1e-3) if opt_kind == "adam" else FusedClipAdam(model.parameters(), lr=1e-3)
    x_i, x_j = (t.to(DEV) for t in synth_clips(4))
    for _ in range(3):
        opt.zero_grad()
        _, _, z_i, z_j = model(x_i, x_j)
        loss = ntxent_loss(z_i, z_j, GRAFP_CFG)
        loss.backward()
        opt.step()
    torch.cuda.synchronize()
    assert torch.isfinite(loss)
    for n, t in model.state_dict().items():
        if not n.startswith(LIVE):
            assert torch.equal(t, before[n]), n                         # unused blocks: parameters AND statistics
        elif n.endswith("num_batches_tracked"):
            assert int(t) == int(before[n]) + 6, n                      # two views x three steps
        elif n in params and n not in BIAS_BEFORE_BN:
            assert not torch.equal(t, before[n]), n                     # the live network trains
    if opt_kind == "adam":
        assert all(p.grad is None for n, p in model.named_parameters() if not n.startswith(LIVE))


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_pipeline_consumers(dt, tmp_path, restore):
    from synth import synth_clips
    from neuralsampleid_amd import downstream, fpdb
    from neuralsampleid_amd.classifier import CrossAttentionClassifier
    from neuralsampleid_amd.fingerprint import GraphedFingerprinter, extract_fingerprints
    model = _model(dt=dt).eval()
    x = synth_clips(6)[0].to(DEV)
    with torch.no_grad():
        nodes, h = model.encoder(model.peak_extractor(x), return_pre_proj=True)
        z = model._project(h)
    assert maxerr(extract_fingerprints(model, x, batch=6).cpu(), z.cpu()) == 0.0
    assert maxerr(GraphedFingerprinter(model, micro_batch=6)(x).cpu(), z.cpu()) == 0.0
    shapes = fpdb.build_node_matrices(model, [("a", x[:4]), ("b", x[4:])], str(tmp_path), batch=4)
    assert shapes == {"a": (4, 512, 32), "b": (2, 512, 32)}
    with torch.no_grad():
        n4, _ = model.encoder(model.peak_extractor(x[:4]), return_pre_proj=True)
    assert np.array_equal(np.load(tmp_path / "a.npy"), n4.float().cpu().numpy())
    n_i, n_j, z_i, z_j = downstream.encode_pairs(model, x, x)
    assert torch.equal(n_i, nodes.float()) and torch.equal(n_j, nodes.float())
    assert torch.equal(z_i, z) and torch.equal(z_j, z)
    torch.manual_seed(0)
    clf = CrossAttentionClassifier(512, num_nodes=32).to(DEV).eval()
    with torch.no_grad():
        s = clf.pair_scores(n_i[:3].contiguous(), n_j[3:].contiguous())
    assert s.shape == (3, 3) and bool(((s > 0) & (s < 1)).all())


def test_eval_reproducible_bitwise(restore):
    from synth import synth_clips
    x = synth_clips(8)[0].to(DEV)
    for dt in (torch.float32, torch.bfloat16):
        model = _model(dt=dt).eval()
        with torch.no_grad():
            a = model.encoder(model.peak_extractor(x), return_pre_proj=True)
            b = model.encoder(model.peak_extractor(x), return_pre_proj=True)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_graphed_train_step_refused(restore):
    from synth import GRAFP_CFG, synth_clips
    from neuralsampleid_amd.graphs import GraphedTrainStep
    from neuralsampleid_amd.optim import FusedClipAdam
    model = _model()
    opt = FusedClipAdam(model.parameters())
    x_i, x_j = (t.to(DEV) for t in synth_clips(4))
    with pytest.raises(NotImplementedError, match="DGL passthrough"):
        GraphedTrainStep(model, opt, GRAFP_CFG, x_i, x_j)
