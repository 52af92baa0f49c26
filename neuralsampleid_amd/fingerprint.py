"""Forward-only fingerprint extraction (the reference's generate.py path, :31-49, :68-100 — BASELINE config 5).

generate.py builds SimCLR(GraphEncoder(k=3)), feeds each audio's (S, 64, 128) log-mel segments through `model(x, x)` in
splits of 128 and keeps z_i. Differences here, all deliberate and documented in DESIGN.md:
  * eval-mode BatchNorm (running statistics) — generate.py never calls model.eval() (test_fp.py:315 does);
  * one view, not two: `model(x, x)` computes the same embedding twice;
  * every split's embeddings are kept (generate.py:44-48 appends only the last one);
  * larger micro-batches (default 1024) and contiguous sharding over ranks with no collective."""
from typing import Tuple

import torch


def shard_bounds(n: int, rank: int, world: int) -> Tuple[int, int]:
    """contiguous clip range [lo, hi) of `rank`; the first n % world ranks take one extra clip"""
    base, extra = divmod(n, world)
    lo = rank * base + min(rank, extra)
    return lo, lo + base + (1 if rank < extra else 0)


def embedding_dim(model) -> int:
    """width of the fingerprints `model._embed` returns: the projector's last layer (SimCLR), or the encoder's embedding head when
    the projector is the identity (simclr/triplet.py BaselineModel: 2048)"""
    proj = model.projector
    if isinstance(proj, torch.nn.Sequential):
        return proj[-1].out_features
    return model.encoder.embedding_head.out_features


def input_shape(model) -> Tuple[int, int]:
    """(bins, frames) of one segment: (n_mels, n_frames) of the cfg for the log-mel models, (84, n_frames) for the baseline's CQT
    segments (config/resnet_ibn.yaml: 216 frames)"""
    from .encoder.resnet_ibn import N_BINS, ResNetIBN
    cfg = model.cfg
    if isinstance(model.encoder, ResNetIBN):
        return N_BINS, int(cfg.get("n_frames", 216))
    return cfg["n_mels"], cfg["n_frames"]


@torch.no_grad()
def extract_fingerprints(model, specs: torch.Tensor, batch: int = 1024, out: torch.Tensor = None) -> torch.Tensor:
    """specs (S, n_mels, n_frames) fp32 on the GPU -> (S, d) L2-normalised fingerprints (fp32).
    The model is run in eval mode (restored afterwards)."""
    was_training = model.training
    model.eval()
    from . import functional, ops
    if functional.ACT_DTYPE == torch.bfloat16:
        ops.register_weight_shadows(model)          # bf16 copies of the weights, converted once (version-checked)
    try:
        S = specs.shape[0]
        d = embedding_dim(model)
        if out is None:
            out = torch.empty((S, d), device=specs.device, dtype=torch.float32)
        for lo in range(0, S, batch):
            hi = min(S, lo + batch)
            _, z = model._embed(specs[lo:hi].contiguous())
            out[lo:hi].copy_(z)
        return out
    finally:
        model.train(was_training)


# The caller's stream is one of the replay lanes (it would otherwise idle while the side streams work). Measured on 100 000 clips,
# one box, two repetitions (k clips/s): 1 lane 386; 2 side streams 380-385, caller + 1 side stream 413; 3 side 400, caller + 2 side 403;
# 4 side 408-410, caller + 3 side 408 — two lanes with the caller's stream among them is the best shape, and bench.py's default.
USE_CALLER_STREAM = True


class GraphedFingerprinter:
    """Forward-only extraction of FULL micro-batches as one hipGraph replay each: a micro-batch is ~130 kernel launches of
    10-90 us, so on a slow host the eager Python loop (not the GPU) sets the rate (round 2, MI355X boxes: 4.1 ms per
    micro-batch of 512 AND of 1024 clips eagerly; 3.5 ms per 1024 clips once the host is out of the way).

        fp = GraphedFingerprinter(model, micro_batch=1024)     # eval mode, captures once (weights are read in place)
        z = fp(specs)                                          # (S, n_mels, n_frames) -> (S, d); a ragged tail is padded

    streams > 1: that many captures of the same forward, each with its own static buffers, replayed on their own HIP streams with
    the micro-batches dealt round-robin — the latency-bound kernels of one micro-batch (one workgroup per clip in the graph builder,
    the small-tile GEMMs of the first stage) run beside the bandwidth-bound ones of another. Measured on MI355X (round 3, 98 304
    clips, micro-batch 2 048): 305.7 k clips/s on one stream, 333.1 k on two, 349.6 k on three; results are identical (same kernels
    on the same data, no cross-stream reduction).

    The captured kernels read the weights and the folded conv+BatchNorm constants in place: after a change of the weights
    (training steps, load_state_dict, torch.optim, in-place edits) build a new GraphedFingerprinter — a call after such a change is
    REFUSED: the guard compares the library's state epochs (writes made by our own kernels behind torch's back) AND the
    (data_ptr, _version) of every parameter and buffer (torch-side writes). The constants the replayed kernels read (folded weights,
    eval affines, bf16 shadows) are referenced from here, so a later eager forward that rebuilds the caches cannot free them under
    the graph."""

    def __init__(self, model, micro_batch: int = 1024, example: torch.Tensor = None, streams: int = 1):
        from . import functional, ops
        self.model, self.mb = model, int(micro_batch)
        dev = next(model.parameters()).device
        cfg = model.cfg
        shape = (self.mb,) + (input_shape(model) if example is None else tuple(example.shape[1:]))
        self.n_streams = max(1, int(streams))
        self.xs = [torch.zeros(shape, device=dev) for _ in range(self.n_streams)]
        self.x = self.xs[0]
        self.d = embedding_dim(model)
        self.epochs = (ops.WEIGHT_EPOCH, ops.STATS_EPOCH)
        self._held = None
        was_training = model.training
        model.eval()
        try:
            with torch.no_grad():
                if functional.ACT_DTYPE == torch.bfloat16:
                    ops.register_weight_shadows(model)
                side = torch.cuda.Stream(device=dev)
                side.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(side):
                    for _ in range(2):            # builds every cached constant (folded weights, shadows) outside the capture
                        model._embed(self.x)
                torch.cuda.current_stream().wait_stream(side)
                torch.cuda.synchronize()
                self.graphs, self.zs = [], []
                for x_s in self.xs:
                    g = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(g):
                        _, z_s = model._embed(x_s)
                    self.graphs.append(g)
                    self.zs.append(z_s)
                self.graph, self.z = self.graphs[0], self.zs[0]
                self.streams = [torch.cuda.Stream(device=dev) for _ in range(self.n_streams)] if self.n_streams > 1 else []
                # everything the captured kernels read in place, kept alive with the graph
                self._held = (list(ops._FOLDED.values()), list(ops._EVAL_AFFINE.values()),
                              [e[0] for e in ops.SHADOWS.entries.values()])
                self._versions = self._state_versions()
        finally:
            model.train(was_training)

    def _state_versions(self):
        # the tensor list is fixed by the capture (the replayed kernels read THESE tensors in place). Per call the guard makes ONE pass
        # over the cached slots (module dict, name, tensor): plain dict look-ups, no module-tree walk, no attribute protocol
        # (~450 slots, tens of microseconds in front of a ~5 ms replay)
        if getattr(self, "_state_slots", None) is None:
            slots = []
            for m in self.model.modules():
                for d in (m._parameters, m._buffers):
                    for name, t in d.items():
                        if t is not None:
                            slots.append((d, name, t))
            self._state_slots = slots
            self._state_modules = [(m, len(m._parameters), len(m._buffers), len(m._modules)) for m in self.model.modules()]
            self._state_children = [(m._modules, name, c) for m in self.model.modules() for name, c in m._modules.items()]
        return tuple((t.data_ptr(), t._version) for _, _, t in self._state_slots)

    def _state_changed(self) -> bool:
        for (d, name, t), (ptr, ver) in zip(self._state_slots, self._versions):
            # a parameter or buffer REPLACED in its module (load_state_dict(assign=True), model.x = nn.Parameter(...), parametrize) is a
            # different object in the module's dict: the captured kernels still read the old tensor
            if d.get(name) is not t or t._version != ver or t.data_ptr() != ptr:
                return True
        for d, name, c in self._state_children:            # a sub-module swapped for another one
            if d.get(name) is not c:
                return True
        for m, n_p, n_b, n_m in self._state_modules:       # tensors or sub-modules added / removed since the capture
            if len(m._parameters) != n_p or len(m._buffers) != n_b or len(m._modules) != n_m:
                return True
        return False

    @torch.no_grad()
    def __call__(self, specs: torch.Tensor, out: torch.Tensor = None) -> torch.Tensor:
        from . import ops
        if (ops.WEIGHT_EPOCH, ops.STATS_EPOCH) != self.epochs or self._state_changed():
            raise RuntimeError("the model's weights or running statistics changed since this graph was captured: "
                               "build a new GraphedFingerprinter")
        S = specs.shape[0]
        if out is None:
            out = torch.empty((S, self.d), device=specs.device, dtype=torch.float32)
        # a ragged tail rides through the same graph: its clips overwrite the head of a static input buffer, the rows behind them
        # keep the previous micro-batch's clips (eval mode: every clip is independent), and only the tail's rows are copied out.
        # COST: a tail of any length is a whole micro-batch of work (a 1-clip tail = micro_batch clips of compute); callers with many
        # short calls should size micro_batch to their call, or batch their clips before calling.
        bounds = [(lo, min(lo + self.mb, S)) for lo in range(0, S, self.mb)]
        if self.n_streams == 1 or len(bounds) == 1:
            for lo, hi in bounds:
                self.x[:hi - lo].copy_(specs[lo:hi], non_blocking=True)
                self.graph.replay()
                out[lo:hi].copy_(self.z[:hi - lo], non_blocking=True)
        else:
            cur = torch.cuda.current_stream()
            ready = torch.cuda.Event()
            ready.record(cur)                                    # specs / out as the caller's stream left them
            lanes = ([cur] + self.streams[1:]) if USE_CALLER_STREAM else self.streams
            for st in lanes:
                if st is not cur:
                    st.wait_event(ready)
            for i, (lo, hi) in enumerate(bounds):
                s_ = i % self.n_streams
                with torch.cuda.stream(lanes[s_]):               # in-order within a stream: the static buffers are reused safely
                    self.xs[s_][:hi - lo].copy_(specs[lo:hi], non_blocking=True)
                    self.graphs[s_].replay()
                    out[lo:hi].copy_(self.zs[s_][:hi - lo], non_blocking=True)
            for st in lanes:
                if st is not cur:
                    cur.wait_stream(st)
        return out


@torch.no_grad()
def fingerprints_from_waveform(model, front, wave: torch.Tensor, batch: int = 1024) -> torch.Tensor:
    """mono fp32 waveform on the GPU -> (S, d) fingerprints: log-mel front end (frontend.LogMelFrontEnd, the reference's
    MelSpectrogram + AmplitudeToDB + 87.5 %-overlap unfold) fused ahead of the encoder — SURVEY.md §8f-4."""
    segs = front(wave)
    if segs.shape[0] == 0:
        return torch.empty((0, embedding_dim(model)), device=wave.device)
    return extract_fingerprints(model, segs, batch)
