"""Times the DGL-variant passthrough encoder (encoder/dgl/passthrough.py: the network the reference's GraphEncoderDGL actually
computes) on one GPU, next to a torch-eager restatement of the same live network written here, on the same GPU.

    python tools/dgl_passthrough_bench.py [--batch 256] [--clips 100000] [--reps 7] [--only-ours]

Per activation storage (fp32: the reference's arithmetic; bf16 storage, fp32 accumulate):
  train_ms  : one contrastive step at --batch (both views forward, NT-Xent, backward, optimiser): the HIP path with
              optim.FusedClipAdam, the eager restatement with torch.optim.Adam; median of --reps after two warm-up steps, device
              events around each step;
  clips_s   : fingerprint extraction over --clips clips (GraphedFingerprinter, micro-batch 1024; eager: the restatement under
              torch.no_grad, same micro-batch), wall time of the whole pass ending in a device synchronise.
One JSON line per storage type. --only-ours skips the eager runs (a rocprofv3 --kernel-trace --stats run uses it)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests", "golden")):
    if p not in sys.path:
        sys.path.insert(0, p)
from synth import GRAFP_CFG  # noqa: E402
from neuralsampleid_amd import functional as F_  # noqa: E402
from neuralsampleid_amd.encoder.dgl.passthrough import PassthroughGraphEncoderDGL  # noqa: E402
from neuralsampleid_amd.fingerprint import GraphedFingerprinter  # noqa: E402
from neuralsampleid_amd.optim import FusedClipAdam  # noqa: E402
from neuralsampleid_amd.simclr.ntxent import ntxent_loss  # noqa: E402
from neuralsampleid_amd.simclr.simclr import SimCLR  # noqa: E402

MB = 1024


class EagerLive(nn.Module):
    """the live network of SimCLR(GraphEncoderDGL) in plain torch, on copies of a passthrough model's weights: peak extractor
    (per-clip min-max normalisation, time / frequency ramps, patch conv, ReLU), stem, three Downsample layers, proj, node mean,
    projector, L2 normalisation"""

    def __init__(self, model, dtype):
        super().__init__()
        enc, cfg = model.encoder, model.cfg
        self.pb, self.pf = cfg["patch_bins"], cfg["patch_frames"]
        self.peak = nn.Conv2d(3, cfg["n_filters"], (self.pb, self.pf), stride=(self.pb, self.pf))
        self.peak.load_state_dict({k[len("convs.0."):]: v for k, v in model.peak_extractor.state_dict().items()})
        self.stem = nn.Sequential(nn.Conv2d(enc.stem[0].in_channels, enc.channels[0], 1, bias=False), nn.BatchNorm2d(enc.channels[0]),
                                  nn.LeakyReLU(0.2))
        self.stem.load_state_dict(enc.stem.state_dict())
        self.ds = nn.ModuleList()
        for d in enc.downsamples():
            m = nn.Sequential(nn.Conv1d(d.conv[0].in_channels, d.conv[0].out_channels, 3, stride=2, padding=1),
                              nn.BatchNorm1d(d.conv[0].out_channels), nn.ReLU())
            m.load_state_dict(d.conv.state_dict())
            self.ds.append(m)
        self.proj = nn.Conv2d(enc.channels[-1], enc.emb_dims, 1)
        self.proj.load_state_dict(enc.proj.state_dict())
        self.projector = nn.Sequential(nn.Linear(cfg["h"], cfg["d"] * cfg["u"]), nn.ELU(), nn.Linear(cfg["d"] * cfg["u"], cfg["d"]))
        self.projector.load_state_dict(model.projector.state_dict())
        self.to(next(model.parameters()).device, dtype)

    def embed(self, x):
        B, H, W = x.shape
        lo, hi = x.amin(dim=(1, 2), keepdim=True), x.amax(dim=(1, 2), keepdim=True)
        s = (x - lo) / (hi - lo)
        t = torch.linspace(0, 1, W, device=x.device, dtype=x.dtype).view(1, 1, W).expand(B, H, W)
        f = torch.linspace(0, 1, H, device=x.device, dtype=x.dtype).view(1, H, 1).expand(B, H, W)
        y = F.relu(self.peak(torch.stack((t, f, s), dim=1)))
        y = self.stem(y.flatten(2).unsqueeze(-1)).squeeze(-1)
        for m in self.ds:
            y = m(y)
        h = self.proj(y.unsqueeze(-1)).mean(dim=2).squeeze(-1)
        return F.normalize(self.projector(h), p=2, dim=1, eps=1e-10)


def ntxent_eager(z_i, z_j, tau):
    """simclr/ntxent.py's loss, vectorised: rows interleaved (z_i[0], z_j[0], ...), self-similarity dropped, the partner's log-softmax"""
    z = torch.stack((z_i, z_j), dim=1).reshape(2 * z_i.shape[0], z_i.shape[1])
    a = (z @ z.T / tau).fill_diagonal_(float("-inf"))
    idx = torch.arange(z.shape[0], device=z.device)
    return -F.log_softmax(a, dim=1)[idx, idx ^ 1].mean()


def clips(n, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return torch.randn(n, GRAFP_CFG["n_mels"], GRAFP_CFG["n_frames"], device="cuda", generator=g) * 20.0 - 40.0


def timed(fn, reps):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return float(np.median(ms)), [round(m, 3) for m in ms]


def rate(fn, n):
    fn(n // 10)                 # warm-up: allocator, code objects, cached constants
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn(n)
    torch.cuda.synchronize()
    return n / (time.perf_counter() - t0)


def model_for(dt):
    F_.set_activation_dtype(dt)
    torch.manual_seed(0)
    return SimCLR(GRAFP_CFG, PassthroughGraphEncoderDGL(cfg=GRAFP_CFG, in_channels=GRAFP_CFG["n_filters"], k=3, size="t")).cuda()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--clips", type=int, default=100_000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--only-ours", action="store_true")
    args = ap.parse_args()
    B = args.batch
    x_i = clips(B, 1)
    x_j = x_i + 3.0 * clips(B, 2)
    specs = clips(args.clips, 3)
    for name, dt in (("fp32", torch.float32), ("bf16", torch.bfloat16)):
        model = model_for(dt).train()
        eager_src = {k: v.clone() for k, v in model.state_dict().items()}
        opt = FusedClipAdam(model.parameters(), lr=GRAFP_CFG["lr"])

        def step():
            opt.zero_grad()
            _, _, z_i, z_j = model(x_i, x_j)
            ntxent_loss(z_i, z_j, GRAFP_CFG).backward()
            opt.step()

        ms, ms_all = timed(step, args.reps)
        model.load_state_dict(eager_src)
        model.eval()
        gf = GraphedFingerprinter(model, micro_batch=MB)
        rec = {"storage": name, "batch": B, "hip_train_ms": round(ms, 3), "hip_train_all": ms_all,
               "hip_clips_s": round(rate(lambda n: gf(specs[:n]), args.clips), 0), "clips": args.clips}
        del gf
        F_.DIRECT_GRADS = False
        if not args.only_ours:
            eager = EagerLive(model, dt).train()
            eopt = torch.optim.Adam(eager.parameters(), lr=GRAFP_CFG["lr"])

            def estep():
                eopt.zero_grad()
                loss = ntxent_eager(eager.embed(x_i.to(dt)).float(), eager.embed(x_j.to(dt)).float(), GRAFP_CFG["tau"])
                loss.backward()
                torch.nn.utils.clip_grad_norm_(eager.parameters(), max_norm=1.0)
                eopt.step()

            ems, ems_all = timed(estep, args.reps)
            eager.eval()

            @torch.no_grad()
            def eextract(n):
                out = torch.empty((n, GRAFP_CFG["d"]), device="cuda")
                for lo in range(0, n, MB):
                    out[lo:lo + MB] = eager.embed(specs[lo:min(n, lo + MB)].to(dt)).float()
                return out

            rec.update({"eager_train_ms": round(ems, 3), "eager_train_all": ems_all,
                        "eager_clips_s": round(rate(eextract, args.clips), 0)})
            rec["train_speedup"] = round(ems / ms, 2)
            rec["extract_speedup"] = round(rec["hip_clips_s"] / rec["eager_clips_s"], 2)
        print(json.dumps(rec), flush=True)
        del model, opt
        torch.cuda.empty_cache()
    F_.set_activation_dtype(torch.float32)


if __name__ == "__main__":
    main()
