"""Which songs does this query sample? A resident index on the GPU: search, song-level vote and classifier re-rank without files.

    idx = SampleIndex(model, classifier=clf, front=LogMelFrontEnd(cfg))
    idx.add_dummy(noise_fp)                               # optional: rows that can be retrieved but never vote
    for name, specs in songs:
        idx.add(name, specs=specs)                        # or wave=..., or add_rows(name, fp, nodes) from fpdb files
    r = idx.identify(wave=query, k_probe=20, top=10)      # r.songs: names, best first; r.totals; r.n_songs
    r = idx.identify(specs=q_specs, rerank=True)          # the stage-2 classifier decides

Reference: the votes are eval.py:296-367 (sequence scores, search.aggregate_hit_rates's rule) and eval_hr.py:85-156 (classifier
scores, rerank.vote_hit_rates_clf's rule), on csrc/vote.hip; match_score and rejection_stats are ablation.py:84-97 and :111-139.
The fingerprints live in a FlatL2Index over dummy ++ ref, the candidates' projected [K | P] classifier rows (4 N (C + 512) bytes
per reference segment) and the song codes next to it, so an identification is search -> scores -> vote on the device and only
the `top` results come back. The file-based evaluations (search.eval_hit_rates, rerank.eval_hit_rates_clf) are unchanged and do
not use this module.

Where in time: align / locate answer "song X, query rows i0..i1, taken from song rows j0..j1, played about `stretch` times as fast"
with a local alignment of the query's rows against a song's rows (csrc/align.hip; the rule is stated in include/nsid.h). The
reference has no such step (eval.py:250-258 leaves it to "future implementations"); sample100-ext's per-occurrence annotations are
what interval_recall is shaped for.

    occs = idx.locate(wave=query, threshold=0.6, min_score=2.0)      # [Occurrence(song, score, q_rows, r_rows, q_time, r_time, stretch)]
    per_song = idx.align(q_fp, ["song a", "song b"], threshold=0.6)

A query that is already in the index: leave_out= keeps the named song's rows out of the search itself (exclude= only keeps it out of
the vote, after its rows took the k_probe slots), and links runs every song against all the others that way, batched.

    occs = idx.locate(fp=idx.fingerprints[lo:lo + n], leave_out="song a", threshold=0.6, min_score=2.0)
    res = idx.links(threshold=0.6, min_score=2.0)                    # res.occurrences[name], res.skipped

A recording of any length (a mix, a broadcast): scan / scanner run the same alignment in windows, the last two rows of every open
song carried from window to window, so an occurrence that crosses a window boundary is found once, in rows of the whole recording.

    occs = idx.scan(wave=recording, threshold=0.6, min_score=2.0)
    sc = idx.scanner(threshold=0.6, min_score=2.0); sc.push(fp_piece); ...; occs = sc.finish()

Which songs are aligned is decided by window votes. The default is the reference's sequence score, which sees an excerpt only where
it starts a window; vote="diagonal" on locate / scan / links votes by the histogram of the hits' diagonals instead (csrc/diag_vote.hip,
the score eval.py:249-258 leaves to "future implementations"), which sees it anywhere in the window; diag_votes is that vote alone.

    occs = idx.scan(wave=recording, threshold=0.6, min_score=2.0, vote="diagonal")

Songs of more than 4096 rows (about 35 minutes: a mix, a live set, an audiobook chapter) are columns of the alignment only in an index
made with long_songs=True, up to 16384 rows (2 h 19 min; the bound under which a cell of the walk keeps its 8 bytes, include/nsid.h
nsid_local_align_panels). The walk then goes over the song in panels of 4096 columns and over a long query in strips of 4096 rows.

    idx = SampleIndex(model, long_songs=True)

The alignment behind an occurrence's four corners: paths traces every occurrence back to its row-by-row mapping (which song row is
query row i? a tempo estimate over all cells; how straight the path is), recomputed from the occurrence's own box, bit for bit the
path of the walk that found it (include/nsid.h nsid_align_paths).

    paths = idx.paths(q_fp, occs, threshold=0.6)                     # [AlignmentPath]: q_rows, r_rows, scores, slope, song_row(...)

Not here: the MAP rule (rerank.vote_map_clf), audio decoding, a command line, sharding over GPUs; songs past 16384 rows (past 4096
without long_songs), queries past that outside scan (refused, not split), rerank=True against a song past 4096 rows, gap steps other
than (1,1), (1,2), (2,1), hipGraph capture of the alignment, an alignment threshold calibrated on real audio, parsing sample100-ext's
annotation files; paths of rerank=True occurrences, of occurrences past 4096 rows on a side, and a Scanner that keeps its rows for
paths (the caller passes the recording's rows)."""
from typing import List, NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch

from . import ops
from .search import FlatL2Index

PROJ_BLOCK = 4096             # segments per classifier projection call
CLF_THRESHOLD = 0.5           # eval_hr.py:131


class Identification(NamedTuple):
    songs: List[str]          # names, best first (at most `top`)
    totals: np.ndarray        # float64, one per name
    n_songs: int              # the distinct songs that voted (can exceed `top`)


class PairVotes:
    """the votes of many (start, length) pairs: device tensors codes (pairs, top) int32 (-1 past the last song), totals (pairs, top)
    float64, n_songs (pairs,) int32; with a re-rank also the flat classifier scores and, per pair, the offset and the row length of
    its block (column j = walk position j)"""

    def __init__(self, names, codes, totals, n_songs, scores=None, s_off=None, s_ld=None):
        self.names, self.codes, self.totals, self.n_songs = names, codes, totals, n_songs
        self.scores, self.s_off, self.s_ld = scores, s_off, s_ld

    def __len__(self):
        return self.codes.shape[0]

    def results(self) -> List[Identification]:
        codes, totals, n = self.codes.cpu().numpy(), self.totals.cpu().numpy(), self.n_songs.cpu().numpy()
        out = []
        for p in range(codes.shape[0]):
            m = int((codes[p] >= 0).sum())
            out.append(Identification([self.names[c] for c in codes[p, :m].tolist()], totals[p, :m].copy(), int(n[p])))
        return out


class DiagIdentification(NamedTuple):
    songs: List[str]          # names, best first (at most `top`)
    counts: np.ndarray        # int32: the hits in each song's best diagonal bin
    q_rows: np.ndarray        # (songs, 2) int32: first and last row of the query table among those hits
    r_rows: np.ndarray        # (songs, 2) int32: first and last reference row (index order, dummies not counted) among them
    n_songs: int              # the distinct songs that voted (can exceed `top`)


class DiagVotes:
    """the diagonal-histogram votes of many (start, length) pairs (ops.diag_vote): device tensors codes, counts, i_lo, i_hi, r_lo, r_hi
    (pairs, top) int32 (-1, or 0 for counts, past the last song) and n_songs (pairs,) int32"""

    def __init__(self, names, codes, counts, i_lo, i_hi, r_lo, r_hi, n_songs):
        self.names, self.codes, self.counts, self.n_songs = names, codes, counts, n_songs
        self.i_lo, self.i_hi, self.r_lo, self.r_hi = i_lo, i_hi, r_lo, r_hi

    def __len__(self):
        return self.codes.shape[0]

    def results(self) -> List[DiagIdentification]:
        codes, counts, n = self.codes.cpu().numpy(), self.counts.cpu().numpy(), self.n_songs.cpu().numpy()
        q = torch.stack([self.i_lo, self.i_hi], dim=2).cpu().numpy()
        r = torch.stack([self.r_lo, self.r_hi], dim=2).cpu().numpy()
        out = []
        for p in range(codes.shape[0]):
            m = int((codes[p] >= 0).sum())
            out.append(DiagIdentification([self.names[c] for c in codes[p, :m].tolist()], counts[p, :m].copy(), q[p, :m].copy(),
                                          r[p, :m].copy(), int(n[p])))
        return out


VOTES = ("sequence", "diagonal")
DIAG_BIN_ROWS = 16            # no measurement on real audio stands behind it: an excerpt of up to 64 rows at 1.25x drifts 16 rows
DIAG_MIN_HITS = 2             # nor behind this: one hit is no diagonal


def _vote_options(what, vote, bin_rows, min_hits, rerank=False, norm_search=False):
    """the refusals of the vote keywords, before anything is launched; returns (vote, bin_rows, min_hits)"""
    if vote not in VOTES:
        raise ValueError(f"{what}: vote = {vote!r} is not one of {VOTES}")
    if norm_search and rerank:
        raise ValueError(f"{what}: norm_search=True is not offered with rerank=True: the re-rank's candidates come from the L2 search")
    if norm_search and vote != "diagonal":
        raise ValueError(f"{what}: norm_search=True needs vote='diagonal': the sequence vote sums per song, and a song with many "
                         "generic rows wins it under normalised scores as well (there is no normalised sequence vote)")
    if vote == "diagonal" and rerank:
        raise ValueError(f"{what}: vote='diagonal' counts search hits and has no re-ranked form (the classifier vote is a different "
                         "rule): use vote='sequence' with rerank=True")
    bin_rows, min_hits = int(bin_rows), int(min_hits)
    if not 1 <= bin_rows <= ops.DIAG_MAX_BIN:
        raise ValueError(f"{what}: bin_rows = {bin_rows} is outside [1, {ops.DIAG_MAX_BIN}]")
    if min_hits < 1:
        raise ValueError(f"{what}: min_hits = {min_hits} must be at least 1")
    return vote, bin_rows, min_hits


def _is_baseline(model) -> bool:
    from .encoder.resnet_ibn import ResNetIBN
    return isinstance(model.encoder, ResNetIBN)


def _need_tensor(t, what, dim, shape_text):
    """type, rank and dtype: ValueError / TypeError before the device is looked at"""
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{what}: expected a torch tensor on the GPU")
    if t.dim() != dim:
        raise ValueError(f"{what}: expected {shape_text}, got {tuple(t.shape)}")
    if t.dtype != torch.float32:
        raise ValueError(f"{what}: expected float32, got {t.dtype}")


def _need_cuda(t, what):
    if not t.is_cuda:
        raise RuntimeError(f"{what}: SampleIndex runs on the MI355X (cuda) device; there is no CPU path")


class SampleIndex:
    """A resident sample-identification index. model: SimCLR (graph encoder) or BaselineModel (ResNet-IBN, no re-rank); classifier: a
    CrossAttentionClassifier for rerank=True and match_score; front: LogMelFrontEnd / CQTFrontEnd, needed only for waveforms.
    model may be None for an index fed with precomputed rows only (add_rows, identify(fp=...)); then d is taken from the first
    rows. prefilter: the index's searches (identify, identify_pairs, locate, links) run through FlatL2Index's certified bf16
    pre-filter; the results are the same bits. long_songs: align, locate, scan / scanner and links take resident songs of up to
    ops.ALIGN_MAX_SONG_ROWS rows as columns (align / locate also such queries, links such songs as queries) instead of
    ops.ALIGN_MAX_COLS; False is the behaviour without the argument in every respect."""

    def __init__(self, model, classifier=None, front=None, device="cuda", micro_batch: int = 1024, prefilter: bool = False,
                 long_songs: bool = False):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("SampleIndex runs on the MI355X (cuda) device; there is no CPU path")
        self.model, self.classifier, self.front = model, classifier, front
        self.micro_batch = int(micro_batch)
        self.prefilter = bool(prefilter)
        self.long_songs = bool(long_songs)
        # the most rows of a song as the columns, and of a query, of the alignment
        self._max_cols = ops.ALIGN_MAX_SONG_ROWS if self.long_songs else ops.ALIGN_MAX_COLS
        self._max_q = ops.ALIGN_MAX_SONG_ROWS if self.long_songs else ops.ALIGN_MAX_ROWS
        self.names: List[str] = []
        self._code = {}
        self._song_rows = []                  # per song: (first ref row, rows, rows with node matrices)
        self._index: Optional[FlatL2Index] = None       # made with the first rows: nothing touches the device before
        self._d = None
        self.n_dummy = 0
        self.n_ref = 0
        self._song_of = None                  # (capacity,) int32 on the device: song code per ref row
        self._song_of_nodes = None            # the same, -1 for a row without node matrices
        self._kp = None                       # (capacity N, C + 512): the candidates' [K | P] rows
        self.N = None                         # nodes per segment of the resident table
        self._cohort = None                   # (M, d): the cohort of normalize=True, a copy (set_cohort)
        self._stat = None                     # (mu, rs), (capacity,) fp32 each: the cohort statistics of the first _stat_done ref rows
        self._stat_done = 0
        self._istat = None                    # (mu, rs) likewise of the first _istat_done index rows (dummy ++ ref): norm_search=True
        self._istat_done = 0
        if model is not None:
            from .fingerprint import embedding_dim
            self._d = int(embedding_dim(model))

    # ------------------------------------------------------------------------------------------------ state
    @property
    def d(self) -> Optional[int]:
        return self._d

    @property
    def C(self) -> Optional[int]:
        return None if self.classifier is None else int(self.classifier.attn.embed_dim)

    @property
    def fingerprints(self) -> torch.Tensor:
        """the reference rows (n_ref, d) on the device, in add order"""
        return self._index.xb[self.n_dummy:]

    @property
    def kp_bytes_per_segment(self) -> int:
        return 0 if self._kp is None else 4 * self.N * self._kp.shape[1]

    def __contains__(self, name) -> bool:
        return name in self._code

    def code(self, name: str) -> int:
        if name not in self._code:
            raise KeyError(f"SampleIndex: no song named {name!r}")
        return self._code[name]

    def _check_fp(self, fp, what, device=True):
        _need_tensor(fp, what, 2, "(rows, d) fingerprints")
        if self._d is not None and fp.shape[1] != self._d:
            raise ValueError(f"{what}: the index holds d = {self._d} fingerprints, got {tuple(fp.shape)}")
        if not ops.search_d_ok(fp.shape[1]):
            raise ValueError(f"{what}: d = {fp.shape[1]} is outside the search kernels' limits ({ops.SEARCH_D_LIMITS})")
        if device:
            _need_cuda(fp, what)

    def _store(self):
        """the device state, made with the first rows"""
        if self._index is None:
            self._index = FlatL2Index(self._d, self.device, prefilter=self.prefilter)
            self._song_of = torch.empty((0,), device=self.device, dtype=torch.int32)
            self._song_of_nodes = torch.empty((0,), device=self.device, dtype=torch.int32)
        return self._index

    def _check_nodes(self, nodes, what):
        if self.classifier is None:
            raise RuntimeError(f"{what}: node matrices need a classifier (SampleIndex(model, classifier=...))")
        _need_tensor(nodes, what, 3, f"(S, {self.C}, N) node matrices")
        if nodes.shape[1] != self.C:
            raise ValueError(f"{what}: expected (S, {self.C}, N) node matrices for a classifier of in_dim {self.C}, got {tuple(nodes.shape)}")
        if self.N is not None and nodes.shape[2] != self.N:
            raise ValueError(f"{what}: the index holds node matrices of N = {self.N} nodes, got {tuple(nodes.shape)}")
        if not 1 <= nodes.shape[2] <= ops.CLF_MAX_N_EVAL:
            raise ValueError(f"{what}: N = {nodes.shape[2]} nodes is outside [1, {ops.CLF_MAX_N_EVAL}]")
        _need_cuda(nodes, what)

    @staticmethod
    def _grown(t, rows, unit=1):
        """t with room for `rows` units of `unit` rows: capacity doubles, earlier rows are kept"""
        if rows * unit <= t.shape[0]:
            return t
        cap = max(rows, 2 * (t.shape[0] // unit))
        new = torch.zeros((cap * unit,) + tuple(t.shape[1:]), device=t.device, dtype=t.dtype)
        new[: t.shape[0]].copy_(t)
        return new

    # ------------------------------------------------------------------------------------------------ encoding
    @torch.no_grad()
    def _encode(self, specs, want_nodes):
        """(S, bins, frames) segments -> (fingerprints (S, d), node matrices (S, C, N) or None): one eval pass per micro-batch, both
        outputs of forward_rows(..., return_nodes=True) as downstream.encode_pairs takes them"""
        from . import functional
        from .fingerprint import extract_fingerprints
        if self.model is None:
            raise RuntimeError("SampleIndex: specs / wave need a model")
        _need_tensor(specs, "specs", 3, "(S, bins, frames) segments")
        _need_cuda(specs, "specs")
        model = self.model
        if _is_baseline(model) or not want_nodes:
            if want_nodes:
                raise NotImplementedError("the ResNet-IBN baseline has no node matrices: rerank / classifier are not available with it")
            return extract_fingerprints(model, specs, self.micro_batch), None
        was_training = model.training
        model.eval()
        if functional.ACT_DTYPE == torch.bfloat16:
            ops.register_weight_shadows(model)
        try:
            pe = model.peak_extractor
            S = specs.shape[0]
            fp = torch.empty((S, self.d), device=specs.device, dtype=torch.float32)
            nodes = []
            for lo in range(0, S, self.micro_batch):
                x = specs[lo:lo + self.micro_batch].contiguous()
                B, H, W = x.shape
                N = (H // pe.patch_bins) * (W // pe.patch_frames)
                rows, n_last, emb = model.encoder.forward_rows(pe.forward_rows(x), B, N, return_nodes=True)
                nodes.append(functional.from_rows(rows, B, n_last).float().contiguous())
                fp[lo:lo + B].copy_(model._project(emb))
            return fp, (torch.cat(nodes, 0) if len(nodes) > 1 else nodes[0]) if nodes else None
        finally:
            model.train(was_training)

    def _segments(self, specs, wave):
        if (specs is None) == (wave is None):
            raise ValueError("give exactly one of specs and wave")
        if wave is not None:
            if self.front is None:
                raise RuntimeError("SampleIndex: a waveform needs a front end (SampleIndex(model, front=LogMelFrontEnd(cfg)))")
            _need_tensor(wave, "wave", 1, "a mono (samples,) waveform")
            _need_cuda(wave, "wave")
            specs = self.front(wave)
        if specs.shape[0] == 0:
            raise ValueError("no segment: the audio is shorter than one segment")
        return specs

    @torch.no_grad()
    def _project(self, fn, nodes):
        parts = [fn(nodes[a:a + PROJ_BLOCK].contiguous()) for a in range(0, nodes.shape[0], PROJ_BLOCK)]
        return torch.cat(parts) if len(parts) > 1 else parts[0]

    # ------------------------------------------------------------------------------------------------ filling
    def add_dummy(self, fp_rows: torch.Tensor) -> None:
        """rows that can be retrieved but never vote (the reference's dummy_db); before the first add()"""
        self._check_fp(fp_rows, "add_dummy")
        if self.n_ref:
            raise RuntimeError("SampleIndex.add_dummy: dummy rows come before the first song (ids are dummy ++ ref)")
        self._d = int(fp_rows.shape[1])
        self._store().add(fp_rows)
        self.n_dummy += fp_rows.shape[0]

    def add(self, name: str, specs: Optional[torch.Tensor] = None, wave: Optional[torch.Tensor] = None) -> int:
        """one song from its (S, bins, frames) segments, or from its waveform through `front`; returns its number of segments"""
        specs = self._segments(specs, wave)
        fp, nodes = self._encode(specs, self.classifier is not None)
        self.add_rows(name, fp, nodes)
        return int(fp.shape[0])

    def add_rows(self, name: str, fp: torch.Tensor, nodes: Optional[torch.Tensor] = None) -> None:
        """one song from precomputed rows: (S, d) fingerprints and, for the re-rank, (S', C, N) node matrices (fpdb's files). Segments
        without node matrices (nodes=None, or S' < S: the reference's missing / short ref_nmatrix file) are retrieved and vote on
        sequence scores, and are skipped by the classifier vote, as eval_hr.py skips them."""
        self._check_fp(fp, "add_rows", device=False)          # every shape before the device: a refusal names the first thing wrong
        if nodes is not None:
            self._check_nodes(nodes, "add_rows")
        _need_cuda(fp, "add_rows")
        if not isinstance(name, str) or name in self._code:
            raise ValueError(f"SampleIndex.add_rows: a song name must be a new string, got {name!r}")
        S = int(fp.shape[0])
        if S == 0:
            raise ValueError("SampleIndex.add_rows: a song needs at least one segment")
        with_nodes = 0
        if nodes is not None:
            with_nodes = min(S, int(nodes.shape[0]))
        code = len(self.names)
        lo, hi = self.n_ref, self.n_ref + S
        kp = None
        if with_nodes:
            kp = self._project(self.classifier.project_candidates, nodes[:with_nodes].contiguous())
        self._d = int(fp.shape[1])
        self._store().add(fp)
        self._song_of = self._grown(self._song_of, hi)
        self._song_of_nodes = self._grown(self._song_of_nodes, hi)
        self._song_of[lo:hi] = code
        self._song_of_nodes[lo:hi] = -1
        self._song_of_nodes[lo:lo + with_nodes] = code
        if self.classifier is not None and (kp is not None or self._kp is not None):
            if self._kp is None:
                self.N = int(nodes.shape[2])
                self._kp = torch.zeros((0, kp.shape[1]), device=self.device, dtype=torch.float32)
            self._kp = self._grown(self._kp, hi, self.N)
            if kp is not None:
                self._kp[lo * self.N:(lo + with_nodes) * self.N].copy_(kp)
        self.names.append(name)
        self._code[name] = code
        self._song_rows.append((lo, S, with_nodes))
        self.n_ref = hi

    # ------------------------------------------------------------------------------------------------ cohort score normalisation
    def set_cohort(self, rows: Optional[torch.Tensor] = None, size: int = 4096) -> None:
        """The cohort of normalize=True (include/nsid.h, "cohort score normalisation"): unrelated rows against which every row's
        scores are read, ops.COHORT_MIN <= M <= ops.COHORT_MAX of them. rows: an (M, d) device tensor, copied. Without rows:
        M = min(size, n_dummy) of the dummy rows, those at positions floor(m n_dummy / M), copied, so that later adds change nothing.
        One cohort per index; setting it drops the cached statistics of the resident rows and of the index rows."""
        if rows is not None:
            self._check_fp(rows, "set_cohort")
            M = int(rows.shape[0])
            if not ops.COHORT_MIN <= M <= ops.COHORT_MAX:
                raise ValueError(f"set_cohort: a cohort of {M} rows is outside [{ops.COHORT_MIN}, {ops.COHORT_MAX}]")
            cohort = rows.detach().clone().contiguous()
        else:
            size = int(size)
            if not ops.COHORT_MIN <= size <= ops.COHORT_MAX:
                raise ValueError(f"set_cohort: size = {size} is outside [{ops.COHORT_MIN}, {ops.COHORT_MAX}]")
            M = min(size, self.n_dummy)
            if M < ops.COHORT_MIN:
                raise RuntimeError(f"set_cohort: the default cohort needs at least {ops.COHORT_MIN} dummy rows, the index holds "
                                   f"{self.n_dummy}; pass rows=")
            pos = (np.arange(M, dtype=np.int64) * self.n_dummy) // M
            cohort = self._index.xb.index_select(0, torch.from_numpy(pos).to(self.device)).contiguous()
        self._cohort, self._stat, self._stat_done = cohort, None, 0
        self._istat, self._istat_done = None, 0

    def _need_cohort(self, what) -> torch.Tensor:
        """the cohort of a normalize=True or norm_search=True call: the one set, or the default one made now"""
        if self._cohort is None:
            if self.n_dummy < ops.COHORT_MIN:
                raise RuntimeError(f"{what}: normalize=True / norm_search=True needs a cohort and the index holds {self.n_dummy} dummy "
                                   f"rows, fewer than the {ops.COHORT_MIN} of a default one: call set_cohort(rows=...) first")
            self.set_cohort()
        if self._d is not None and self._cohort.shape[1] != self._d:
            raise ValueError(f"{what}: the cohort has d = {self._cohort.shape[1]}, the index d = {self._d}: call set_cohort again")
        return self._cohort

    def cohort_stats(self, fp: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        """(mu, rs) of every row of fp (rows, d) against the index's cohort: device fp32, what normalize=True uses for these rows"""
        self._check_fp(fp, "cohort_stats")
        return ops.cohort_stats(fp.contiguous(), self._need_cohort("cohort_stats"))

    def _resident_stats(self, what):
        """(mu, rs) of the n_ref resident rows: the rows added since the last normalised call are computed now, the others are kept"""
        cohort = self._need_cohort(what)
        if self._stat is None:
            self._stat = tuple(torch.empty((0,), device=self.device, dtype=torch.float32) for _ in range(2))
            self._stat_done = 0
        if self._stat_done < self.n_ref:
            new = ops.cohort_stats(self.fingerprints[self._stat_done:self.n_ref], cohort)
            self._stat = tuple(self._grown(t, self.n_ref) for t in self._stat)
            for t, v in zip(self._stat, new):
                t[self._stat_done:self.n_ref].copy_(v)
            self._stat_done = self.n_ref
        return self._stat[0][: self.n_ref], self._stat[1][: self.n_ref]

    def _index_stats(self, what):
        """(mu, rs) of all index rows, dummy ++ ref, which is what competes in a search (norm_search=True). Kept like the resident
        rows': the dummy rows are computed once, the ref part is copied from _resident_stats (the same bits), and only the rows added
        since the last call are touched."""
        ref = self._resident_stats(what)
        n = self.n_dummy + self.n_ref
        if self._istat is None:
            self._istat = tuple(torch.empty((0,), device=self.device, dtype=torch.float32) for _ in range(2))
            self._istat_done = 0
        if self._istat_done < n:
            self._istat = tuple(self._grown(t, n) for t in self._istat)
            if self._istat_done < self.n_dummy:
                new = ops.cohort_stats(self._index.xb[self._istat_done:self.n_dummy], self._cohort)
                for t, v in zip(self._istat, new):
                    t[self._istat_done:self.n_dummy].copy_(v)
                self._istat_done = self.n_dummy
            for t, v in zip(self._istat, ref):
                t[self._istat_done:n].copy_(v[self._istat_done - self.n_dummy:])
            self._istat_done = n
        return self._istat[0][:n], self._istat[1][:n]

    def _norm_search_checks(self, what):
        """the refusals of norm_search=True that do not depend on the vote keywords, before any search is launched"""
        if self.prefilter:
            raise ValueError(f"{what}: norm_search=True is not offered on a prefilter=True index: the pre-filter certifies L2 keys "
                             "(there is no normalised pre-filter)")
        self._need_cohort(what)

    def _norm(self, what, q, resident_query=False, q_stats=None):
        """ops.pair_sim's norm= for query rows q against the resident rows (resident_query: q is the resident rows themselves;
        q_stats: the query rows' statistics where the call has them already)"""
        ref = self._resident_stats(what)
        if resident_query:
            return ref + ref
        return (ops.cohort_stats(q, self._cohort) if q_stats is None else tuple(q_stats)) + ref

    # ------------------------------------------------------------------------------------------------ asking
    def _query(self, specs, wave, fp, nodes, rerank):
        if fp is None:
            fp, enc_nodes = self._encode(self._segments(specs, wave), rerank)
            nodes = enc_nodes if nodes is None else nodes
        elif specs is not None or wave is not None:
            raise ValueError("give fp (with nodes for a re-rank), or specs, or wave")
        return fp, nodes

    def identify(self, specs=None, wave=None, fp=None, nodes=None, k_probe: int = 20, top: int = 10, exclude: Optional[str] = None,
                 rerank: bool = False, leave_out: Optional[str] = None) -> Identification:
        """the songs a query samples, best first: all its L segments as one pair (0, L). exclude: a song name that never votes (the
        reference skips a ref song named like the query id); its rows still take their k_probe slots of the search. leave_out: a song
        name whose rows do not compete in the search at all (the query is that resident song: its own overlapping rows would fill
        every slot); it never votes and the slots go to the other songs."""
        if rerank:
            self._check_rerank()
        if leave_out is not None:
            self.code(leave_out)
        fp, nodes = self._query(specs, wave, fp, nodes, rerank)
        self._check_fp(fp, "identify")
        pv = self.identify_pairs(fp, [0], [fp.shape[0]], k_probe=k_probe, top=top, exclude=None if exclude is None else [exclude],
                                 rerank=rerank, nodes=nodes, leave_out=None if leave_out is None else [leave_out])
        return pv.results()[0]

    def _check_rerank(self):
        if self.model is not None and _is_baseline(self.model):
            raise NotImplementedError("the ResNet-IBN baseline has no node matrices: rerank=True is not available with it")
        if self.classifier is None:
            raise RuntimeError("SampleIndex: rerank=True needs a classifier (SampleIndex(model, classifier=...))")

    @torch.no_grad()
    def identify_pairs(self, fp: torch.Tensor, starts: Sequence[int], lens: Sequence[int], k_probe: int = 20, top: int = 10,
                       exclude: Optional[Sequence[Optional[str]]] = None, rerank: bool = False,
                       nodes: Optional[torch.Tensor] = None, leave_out: Optional[Sequence[Optional[str]]] = None) -> PairVotes:
        """many (start, length) pairs of one query table at once, the evaluation's form: fp (rows, d); pair p votes over rows
        [starts[p], starts[p] + lens[p]); exclude: per pair a song name or None; nodes (rows, C, N) for rerank=True. Every row is
        searched once, and with a re-rank the pairs of one start share one score block at their longest length. leave_out: per pair a
        song name or None; the named song's rows do not compete in the search of the pair's rows (FlatL2Index.search's exclude). A row
        is still searched once, so the pairs that share a row must name the same song (or all None): ValueError otherwise."""
        self._check_fp(fp, "identify_pairs")
        if rerank:
            self._check_rerank()
            if nodes is None:
                raise ValueError("identify_pairs: rerank=True needs the query's node matrices")
            self._check_nodes(nodes, "identify_pairs")
            if nodes.shape[0] != fp.shape[0]:
                raise ValueError(f"identify_pairs: {fp.shape[0]} fingerprints but {nodes.shape[0]} node matrices")
            if self._kp is None:
                raise RuntimeError("identify_pairs: rerank=True, but no song of the index has node matrices")
        k, top, starts, lens, ex, left = self._pair_args("identify_pairs", fp, starts, lens, k_probe, top, exclude, leave_out)
        npairs = starts.size
        if npairs == 0:
            return PairVotes(self.names, torch.empty((0, top), device=self.device, dtype=torch.int32),
                             torch.empty((0, top), device=self.device, dtype=torch.float64),
                             torch.empty((0,), device=self.device, dtype=torch.int32))
        fp = fp.contiguous()
        _, I = self._index.search(fp, k, exclude=left)
        if not rerank:
            scores = ops.seq_scores(fp, self._index.xb, I, starts, lens, int(lens.max()) * k)
            return PairVotes(self.names, *ops.song_vote(I, scores, starts, lens, self._song_of[: self.n_ref], self.n_dummy, ex, top))
        # one group per distinct start: its rows at the longest length against their own candidates, in walk order
        ustarts, inv = np.unique(starts, return_inverse=True)
        longest = np.zeros(ustarts.size, dtype=np.int64)
        np.maximum.at(longest, inv, lens)
        rows = np.concatenate([np.arange(s, s + n) for s, n in zip(ustarts.tolist(), longest.tolist())])
        rows_dev = torch.from_numpy(rows).to(self.device)
        cidx = ops.vote_candidates(I.index_select(0, rows_dev).contiguous(), self.n_dummy, self.n_ref).reshape(-1)
        q = self._project(self.classifier.project_queries, nodes)
        tail = self.classifier.folded()[4]
        out, off = ops.clf_pair_scores_dev(q, self._kp[: self.n_ref * self.N], self.N, tail, ustarts, longest, longest * k, cidx)
        s_off, s_ld = np.asarray(off)[inv], (longest * k)[inv]
        votes = ops.song_vote_clf(I, out, s_off, s_ld, starts, lens, self._song_of_nodes[: self.n_ref], self.n_dummy, ex,
                                  CLF_THRESHOLD, top)
        return PairVotes(self.names, *votes, scores=out, s_off=s_off, s_ld=s_ld)

    def _pair_args(self, what, fp, starts, lens, k_probe, top, exclude, leave_out):
        """the checks of a table of (start, length) pairs that every vote shares; returns (k, top, starts, lens as int64 numpy, the
        exclude codes or None, the leave-out ranges or None)"""
        k, top = int(k_probe), int(top)
        if not 1 <= k <= ops.SEARCH_MAX_K:
            raise ValueError(f"k_probe = {k} is outside [1, {ops.SEARCH_MAX_K}]")
        if not 1 <= top <= ops.VOTE_MAX_TOP:
            raise ValueError(f"top = {top} is outside [1, {ops.VOTE_MAX_TOP}]")
        starts = np.asarray(starts, dtype=np.int64).reshape(-1)
        lens = np.asarray(lens, dtype=np.int64).reshape(-1)
        if starts.shape != lens.shape:
            raise ValueError(f"{what}: starts and lens differ in length")
        if starts.size and (starts.min() < 0 or lens.min() < 1 or (starts + lens).max() > fp.shape[0]):
            raise ValueError(f"{what}: every pair needs 0 <= start, 1 <= length and start + length <= the rows of fp")
        if starts.size and int(lens.max()) * k > ops.VOTE_MAX_CAND:
            raise ValueError(f"{what}: {int(lens.max())} segments x k_probe = {k} is more than {ops.VOTE_MAX_CAND} candidates per "
                             "vote: lower k_probe or split the query")
        ex = None
        if exclude is not None:
            if len(exclude) != starts.size:
                raise ValueError(f"{what}: exclude must hold one song name (or None) per pair")
            ex = np.asarray([-1 if e is None else self.code(e) for e in exclude], dtype=np.int64)
        left = None if leave_out is None else self._leave_out_ranges(leave_out, starts, lens, int(fp.shape[0]))
        if self.n_ref == 0:
            raise RuntimeError("SampleIndex: the index holds no song")
        return k, top, starts, lens, ex, left

    @torch.no_grad()
    def diag_votes(self, fp: torch.Tensor, starts: Sequence[int], lens: Sequence[int], k_probe: int = 20, top: int = 10,
                   bin_rows: int = DIAG_BIN_ROWS, exclude: Optional[Sequence[Optional[str]]] = None,
                   leave_out: Optional[Sequence[Optional[str]]] = None, norm_search: bool = False, _q_stats=None) -> DiagVotes:
        """The diagonal-histogram vote (include/nsid.h nsid_diag_vote) of many (start, length) pairs of one query table: one search and
        one ops.diag_vote, no seq_scores. A song's count is the largest number of its retrieved rows whose offset to the query row
        falls into one bin of 2 bin_rows rows, so an excerpt votes wherever in the pair's rows it starts, and under a time stretch of
        up to bin_rows rows of drift. fp, starts, lens, exclude, leave_out: identify_pairs'. bin_rows = 16 keeps an excerpt of up to 64
        rows at 1.25x in one bin; no measurement on real audio stands behind the number.

        norm_search=True: the k_probe rows of a query row are those of largest cohort-normalised score (FlatL2Index.search_norm: the
        cell normalize=True aligns on) instead of smallest L2 distance, so a query row with a generic component does not spend its
        slots on the catalogue's generic rows. The vote reads ids only and is the same. The query rows' statistics are one
        ops.cohort_stats, the index rows' (dummy ++ ref) are cached; the cohort is normalize's (set_cohort). Refused on a
        prefilter=True index."""
        self._check_fp(fp, "diag_votes")
        bin_rows = _vote_options("diag_votes", "diagonal", bin_rows, 1)[1]
        if norm_search:
            self._norm_search_checks("diag_votes")
        k, top, starts, lens, ex, left = self._pair_args("diag_votes", fp, starts, lens, k_probe, top, exclude, leave_out)
        if starts.size == 0:
            e = lambda: torch.empty((0, top), device=self.device, dtype=torch.int32)
            return DiagVotes(self.names, e(), e(), e(), e(), e(), e(), torch.empty((0,), device=self.device, dtype=torch.int32))
        fp = fp.contiguous()
        if norm_search:
            x_stats = self._index_stats("diag_votes")
            q_stats = ops.cohort_stats(fp, self._cohort) if _q_stats is None else tuple(_q_stats)
            _, I = self._index.search_norm(fp, k, q_stats + x_stats, exclude=left)
        else:
            _, I = self._index.search(fp, k, exclude=left)
        return DiagVotes(self.names, *ops.diag_vote(I, starts, lens, self._song_of[: self.n_ref], self.n_dummy, ex, bin_rows, top))

    def _window_votes(self, fp, starts, lens, k, top, exclude, leave_out, rerank, nodes, vote, bin_rows, min_hits, norm_search=False,
                      q_stats=None):
        """the votes of some windows on the host: (codes (pairs, top), -1 = none; totals (pairs, top); hints (pairs, top, 4) = i_lo, i_hi,
        r_lo, r_hi, or None). vote='sequence': identify_pairs' totals. vote='diagonal': diag_votes' counts, and a song with fewer than
        min_hits hits in its best bin is no candidate."""
        if vote == "sequence":
            pv = self.identify_pairs(fp, starts, lens, k_probe=k, top=top, exclude=exclude, rerank=rerank, nodes=nodes, leave_out=leave_out)
            return pv.codes.cpu().numpy(), pv.totals.cpu().numpy(), None
        dv = self.diag_votes(fp, starts, lens, k_probe=k, top=top, bin_rows=bin_rows, exclude=exclude, leave_out=leave_out,
                             norm_search=norm_search, _q_stats=q_stats)
        packed = torch.stack([dv.codes, dv.counts, dv.i_lo, dv.i_hi, dv.r_lo, dv.r_hi], dim=2).cpu().numpy()      # one copy
        codes, counts = packed[:, :, 0], packed[:, :, 1]
        return np.where(counts >= min_hits, codes, -1), counts, packed[:, :, 2:]

    def _leave_out_ranges(self, leave_out, starts, lens, rows):
        """identify_pairs' leave_out as FlatL2Index.search's exclude: per row of the query table the index rows (dummy ++ ref ids) of
        the song its pairs leave out, (0, 0) for a row no pair names a song for; None when no pair names one. Host only."""
        if len(leave_out) != starts.size:
            raise ValueError("identify_pairs: leave_out must hold one song name (or None) per pair")
        code = np.asarray([-1 if e is None else self.code(e) for e in leave_out], dtype=np.int64)
        if not (code >= 0).any():
            return None
        pair = np.repeat(np.arange(starts.size), lens)
        row = np.arange(int(lens.sum())) - np.repeat(np.cumsum(lens) - lens, lens) + starts[pair]
        least = np.full(rows, len(self.names), dtype=np.int64)    # the smallest and the largest claim of every row
        most = np.full(rows, -2, dtype=np.int64)                  # -2: no pair claims the row
        np.minimum.at(least, row, code[pair])
        np.maximum.at(most, row, code[pair])
        bad = np.flatnonzero((most > -2) & (least != most))
        if bad.size:
            raise ValueError(f"identify_pairs: row {int(bad[0])} is claimed by pairs with different leave_out: a row is searched once")
        song = np.asarray([(lo, n) for lo, n, _ in self._song_rows], dtype=np.int64).reshape(-1, 2)
        has = most >= 0
        lo = np.where(has, self.n_dummy + song[np.maximum(most, 0), 0], 0)
        return lo, np.where(has, lo + song[np.maximum(most, 0), 1], 0)

    @torch.no_grad()
    def match_score(self, nodes_q: torch.Tensor, name: Optional[str] = None, nodes: Optional[torch.Tensor] = None) -> float:
        """ablation.py:84-97: the mean over the query's segments of the best classifier score over a song's segments. The song is a
        resident one (name) or explicit (S, C, N) node matrices (the reference's torch.randn_like stand-in for 'no song')."""
        if self.classifier is None:
            raise RuntimeError("SampleIndex.match_score needs a classifier (SampleIndex(model, classifier=...))")
        if (name is None) == (nodes is None):
            raise ValueError("match_score: give exactly one of name and nodes")
        self._check_nodes(nodes_q, "match_score")
        if nodes_q.shape[0] == 0:
            raise ValueError("match_score: the query has no segment")
        N = int(nodes_q.shape[2])
        if name is not None:
            lo, _, with_nodes = self._song_rows[self.code(name)]
            if with_nodes == 0:
                raise ValueError(f"match_score: song {name!r} has no node matrices")
            if N != self.N:
                raise ValueError(f"match_score: the index holds node matrices of N = {self.N} nodes, got {N}")
            kp = self._kp[lo * N:(lo + with_nodes) * N]
            n_seg = with_nodes
        else:
            self._check_nodes(nodes, "match_score")
            if nodes.shape[2] != N or nodes.shape[0] == 0:
                raise ValueError("match_score: query and song node counts differ, or the song has no segment")
            kp = self._project(self.classifier.project_candidates, nodes.contiguous())
            n_seg = int(nodes.shape[0])
        q = self._project(self.classifier.project_queries, nodes_q.contiguous())
        Sq = int(nodes_q.shape[0])
        out, _ = self.classifier.score_blocks(q, kp, N, [0], [Sq], np.arange(n_seg), [0], [n_seg])
        return float(out.view(Sq, n_seg).max(dim=1).values.double().mean())


    # ------------------------------------------------------------------------------------------------ locating
    def _row_timing(self, row_hop_s, row_len_s):
        """(row hop, row length) in seconds, from the keywords or the front end; None when neither is known"""
        if (row_hop_s is None) != (row_len_s is None):
            raise ValueError("give row_hop_s and row_len_s together")
        if row_hop_s is not None:
            hop, length = float(row_hop_s), float(row_len_s)
            if not (hop > 0 and length > 0):
                raise ValueError("row_hop_s and row_len_s must be positive")
            return hop, length
        if self.front is not None:
            f = self.front
            return f.step * f.hop / f.fs, f.n_frames * f.hop / f.fs
        return None

    def _align_checks(self, what, fp, songs, threshold, top, nodes, rerank, normalize=False):
        """every refusal of align, before the device is touched for the shapes; returns (song codes, threshold)"""
        if normalize and rerank:
            raise ValueError(f"{what}: normalize=True is not offered with rerank=True: the classifier's cells are probabilities and "
                             "their threshold already has a meaning")
        if rerank:
            self._check_rerank()
        elif threshold is None:
            raise ValueError(f"{what}: threshold has no default for fingerprint scores (the reference has no such number and none has "
                             "been measured on real audio): pass one, or use rerank=True")
        self._check_fp(fp, what, device=False)
        max_q = ops.ALIGN_MAX_ROWS if rerank else self._max_q
        if fp.shape[0] > max_q:
            raise ValueError(f"{what}: a query of {fp.shape[0]} rows is past the limit of {max_q}; longer inputs are refused, "
                             "not split")
        top = int(top)
        if not 1 <= top <= ops.ALIGN_MAX_TOP:
            raise ValueError(f"{what}: top = {top} is outside [1, {ops.ALIGN_MAX_TOP}]")
        if isinstance(songs, str):
            raise TypeError(f"{what}: songs must be a sequence of names, not one string")
        codes = [self.code(s) for s in songs]
        max_cols = ops.ALIGN_MAX_COLS if rerank else self._max_cols          # the classifier's cells go through local_align alone
        for c in codes:
            if self._song_rows[c][1] > max_cols:
                raise ValueError(f"{what}: song {self.names[c]!r} has {self._song_rows[c][1]} rows, past the limit of "
                                 f"{max_cols}; longer inputs are refused, not split")
        if rerank:
            if nodes is None:
                raise ValueError(f"{what}: rerank=True needs the query's node matrices")
            self._check_nodes(nodes, what)
            if nodes.shape[0] != fp.shape[0]:
                raise ValueError(f"{what}: {fp.shape[0]} fingerprints but {nodes.shape[0]} node matrices")
            if self._kp is None:
                raise RuntimeError(f"{what}: rerank=True, but no song of the index has node matrices")
            threshold = CLF_THRESHOLD if threshold is None else threshold
        threshold = float(threshold)
        if threshold != threshold:
            raise ValueError(f"{what}: threshold is NaN")
        _need_cuda(fp, what)
        return codes, threshold

    @torch.no_grad()
    def align(self, fp: torch.Tensor, songs: Sequence[str], threshold: Optional[float] = None, min_score: float = 0.0, top: int = 16,
              nodes: Optional[torch.Tensor] = None, rerank: bool = False, return_rows: bool = False, row_hop_s=None, row_len_s=None,
              s_budget_bytes: int = 1 << 30, normalize: bool = False, _q_stats=None):
        """Where in the query, and where in each named resident song, does the query sample the song? The local alignment of
        include/nsid.h ("locating a sample") of the query's rows against each song's rows, one pair per song, all songs in one
        pair_sim + local_align per chunk; a chunk's score workspace (4 Lq Lr bytes per song) stays under s_budget_bytes.

        threshold: the score a (query row, song row) cell must exceed to extend a path. It has NO default for fingerprint scores: the
        reference has no such number and none has been measured on real audio. With rerank=True the cells are the classifier's scores
        of (query row, song row with node matrices) pairs, the song rows without node matrices are not columns, and threshold defaults
        to CLF_THRESHOLD. Returns a list of Occurrence lists, one per song, best first; with return_rows=True also a dict of the per-row
        tensors and the S used, per chunk: {"chunks": [(codes, S, s_off, s_ld, x_len, row_h, row_j, row_org, row_off, occ, occ_score,
        n_occ), ...]}.

        long_songs: a pair with more than ALIGN_MAX_ROWS query rows or more than ALIGN_MAX_COLS song rows goes through
        local_align_panels in strips of ALIGN_MAX_ROWS query rows chained through the carry, then align_occurrences with its span; the
        workspace is then per strip. Such pairs are reported in chunks of their own, whose tuples are (codes, S, s_off, s_ld, x_len,
        row_h, row_j, row_i0, row_j0, row_off, occ, occ_score, n_occ): the origin unpacked (row_i0, row_j0) where the others have
        row_org, and S, s_off, s_ld as lists with one entry per strip. Refused with rerank=True.

        normalize=True: every cell is cohort-normalised (set_cohort; include/nsid.h, "cohort score normalisation"): the query rows'
        statistics are computed in this call, the resident rows' are cached, and pair_sim stores 0.5 (zq + zx) in place of the dot, so
        threshold, min_score and Occurrence.score are in background sigmas. threshold still has no default: no sigma threshold has
        been measured on real audio either. Refused with rerank=True; without a cohort the default one is taken from the dummy rows."""
        timing = self._row_timing(row_hop_s, row_len_s)
        codes, threshold = self._align_checks("align", fp, songs, threshold, top, nodes, rerank, normalize)
        if normalize:
            self._need_cohort("align")
        Lq, top = int(fp.shape[0]), int(top)
        out: List[List[Occurrence]] = [[] for _ in codes]
        chunks = []
        if Lq == 0 or not codes:
            return (out, {"chunks": chunks}) if return_rows else out
        fp = fp.contiguous()
        if not rerank:
            occ, sc = self._align_pairs(fp, np.zeros(len(codes), np.int64), np.full(len(codes), Lq, np.int64), codes, threshold,
                                        min_score, top, int(s_budget_bytes), chunks if return_rows else None,
                                        self._norm("align", fp, q_stats=_q_stats) if normalize else None)
            for p, c in enumerate(codes):
                for (i0, i1, j0, j1), s in zip(occ[p].tolist(), sc[p].tolist()):
                    if i0 < 0:
                        break
                    out[p].append(_occurrence(self.names[c], s, i0, i1, j0, j1, timing))
            return (out, {"chunks": chunks}) if return_rows else out
        qproj = self._project(self.classifier.project_queries, nodes)
        x_len_all = [self._song_rows[c][2] for c in codes]
        lo = 0
        while lo < len(codes):
            hi, used = lo, 0
            while hi < len(codes) and (hi == lo or used + 4 * Lq * x_len_all[hi] <= int(s_budget_bytes)):
                used += 4 * Lq * x_len_all[hi]
                hi += 1
            part = codes[lo:hi]
            x_start = np.asarray([self._song_rows[c][0] for c in part], dtype=np.int64)
            x_len = np.asarray(x_len_all[lo:hi], dtype=np.int64)
            q_len = np.full(len(part), Lq, dtype=np.int64)
            cand = np.concatenate([np.arange(s, s + n) for s, n in zip(x_start.tolist(), x_len.tolist())]) if x_len.sum() else \
                np.zeros(0, dtype=np.int64)
            S, s_off = self.classifier.score_blocks(qproj, self._kp[: self.n_ref * self.N], self.N, np.zeros(len(part), np.int64),
                                                    q_len, cand, np.cumsum(x_len) - x_len, x_len)
            s_off, s_ld = np.asarray(s_off, dtype=np.int64), x_len
            res = ops.local_align(S, s_off, s_ld, q_len, x_len, threshold, min_score, top)
            occ, sc = res[0].cpu().numpy(), res[1].cpu().numpy()
            for p, c in enumerate(part):
                for (i0, i1, j0, j1), s in zip(occ[p].tolist(), sc[p].tolist()):
                    if i0 < 0:
                        break
                    out[lo + p].append(_occurrence(self.names[c], s, i0, i1, j0, j1, timing))
            chunks.append((part, S, s_off, s_ld, x_len) + tuple(res[3:]) + tuple(res[:3]))
            lo = hi
        return (out, {"chunks": chunks}) if return_rows else out

    def _align_pairs(self, q, q_start, q_len, codes, threshold, min_score, top, budget, chunks=None, norm=None):
        """The alignment of pairs (rows q_start[p] .. + q_len[p] of q, resident song codes[p]) over fingerprint scores, for align and
        links: (occ (pairs, top, 4), occ_score (pairs, top)) on the host. Consecutive pairs go in chunks whose score workspace stays
        under `budget` bytes (one pair is always allowed). A chunk of pairs within ALIGN_MAX_ROWS x ALIGN_MAX_COLS is one pair_sim and
        one local_align; a chunk of longer pairs (long_songs) goes strip by strip of ALIGN_MAX_ROWS query rows, all its pairs in one
        pair_sim and one local_align_panels per strip, the first fresh and the others from the carry, and then through
        align_occurrences with the span 2 (x_len - 1); its workspace is that of one strip. chunks: a list that receives align's
        return_rows tuples. norm: ops.pair_sim's norm= for all rows of q and the resident rows (normalize=True), else None."""
        ref = self.fingerprints
        P = len(codes)
        x_start_all = np.asarray([self._song_rows[c][0] for c in codes], dtype=np.int64)
        x_len_all = np.asarray([self._song_rows[c][1] for c in codes], dtype=np.int64)
        strip_all = np.minimum(q_len, ops.ALIGN_MAX_ROWS)
        long = (q_len > ops.ALIGN_MAX_ROWS) | (x_len_all > ops.ALIGN_MAX_COLS)
        occ_all = np.full((P, top, 4), -1, dtype=np.int32)
        sc_all = np.zeros((P, top), dtype=np.float32)
        lo = 0
        while lo < P:
            hi, used = lo, 0
            while hi < P and long[hi] == long[lo]:
                cells = 4 * int(strip_all[hi]) * int(x_len_all[hi])
                if hi > lo and used + cells > budget:
                    break
                used += cells
                hi += 1
            qs, ql, x_start, x_len = q_start[lo:hi], q_len[lo:hi], x_start_all[lo:hi], x_len_all[lo:hi]
            if not long[lo]:
                S, s_off, s_ld = ops.pair_sim(q, ref, qs, ql, x_start, x_len, norm=norm)
                res = ops.local_align(S, s_off, s_ld, ql, x_len, threshold, min_score, top)
                if chunks is not None:
                    chunks.append((list(codes[lo:hi]), S, s_off, s_ld, x_len) + tuple(res[3:]) + tuple(res[:3]))
            else:
                res, kept = self._align_strips(q, ref, qs, ql, x_start, x_len, threshold, min_score, top, chunks is not None, norm)
                if chunks is not None:
                    chunks.append((list(codes[lo:hi]),) + kept + (x_len,) + tuple(res[3:]) + tuple(res[:3]))
            occ_all[lo:hi], sc_all[lo:hi] = res[0].cpu().numpy(), res[1].cpu().numpy()
            lo = hi
        return occ_all, sc_all

    def _align_strips(self, q, ref, q_start, q_len, x_start, x_len, threshold, min_score, top, keep, norm=None):
        """one chunk of long pairs: ((occ, occ_score, n_occ, row_h, row_j, row_i0, row_j0, row_off), (S, s_off, s_ld lists per strip))"""
        dev, R = q.device, ops.ALIGN_MAX_ROWS
        carry, carry_off = ops.align_carry(x_len, dev, long_songs=True)
        row_off = np.cumsum(q_len) - q_len
        total = int(q_len.sum())
        rows = (torch.empty((total,), device=dev, dtype=torch.float32),) + tuple(
            torch.empty((total,), device=dev, dtype=torch.int32) for _ in range(3))
        kept = ([], [], [])
        for lo in range(0, int(q_len.max()), R):
            n = np.clip(q_len - lo, 0, R)
            on = n > 0
            S, s_off, s_ld = ops.pair_sim(q, ref, q_start[on] + lo, n[on], x_start[on], x_len[on], long_songs=True, norm=norm)
            ops.local_align_panels(S, s_off, s_ld, n[on], x_len[on], threshold, np.full(int(on.sum()), lo, np.int64),
                                   np.full(int(on.sum()), 1 if lo == 0 else 0, np.int64), carry, carry_off[on], rows=rows,
                                   row_off=row_off[on] + lo)
            if keep:
                for u, v in zip(kept, (S, s_off, s_ld)):
                    u.append(v)
        occ = ops.align_occurrences(*rows, row_off, q_len, np.zeros(len(q_len), np.int64), min_score, top,
                                    span=np.maximum(2 * (x_len - 1), 0))
        return tuple(occ) + rows + (row_off,), kept

    @torch.no_grad()
    def locate(self, specs=None, wave=None, fp=None, nodes=None, songs: Optional[Sequence[str]] = None, k_probe: int = 20,
               n_songs: int = 5, exclude: Optional[str] = None, threshold: Optional[float] = None, min_score: float = 0.0,
               top: int = 16, rerank: bool = False, row_hop_s=None, row_len_s=None,
               leave_out: Optional[str] = None, vote: str = "sequence", bin_rows: int = DIAG_BIN_ROWS,
               min_hits: int = DIAG_MIN_HITS, normalize: bool = False, norm_search: bool = False) -> List["Occurrence"]:
        """The occurrences of resident songs in a query, one flat list sorted by score: encodes as identify does, finds the candidate
        songs (songs=None) and aligns the query against them.

        The candidates: the query is cut into consecutive windows of W = min(Lq, VOTE_MAX_CAND // k_probe) rows (the last one ends at
        the last row), one identify_pairs call votes in every window, and the songs of any window's top list are ordered by their best
        window total (descending, then by code); the first n_songs are aligned. This is also what lets a whole track through at
        k_probe = 20. exclude: a song name that is never a candidate. leave_out: a song name whose rows do not compete in the search
        (identify's leave_out: the query is that resident song), so it is never a candidate either and the other songs get its slots;
        refused with songs=, as exclude is. threshold: see align (no default without rerank).

        vote="diagonal": the windows are voted by diag_votes instead (no seq_scores): a window's candidates are its songs with at least
        min_hits hits in one diagonal bin of 2 bin_rows rows, ordered across windows by their best window count, then code. The
        sequence vote scores a candidate against the window's first rows, so it sees an excerpt only where it starts a window; the
        diagonal vote sees it anywhere in the window. Refused with rerank=True. bin_rows and min_hits have no measurement on real
        audio behind them.

        normalize=True: align's (threshold and scores in background sigmas; refused with rerank=True). It is the alignment's flag:
        the candidate search and both votes run on L2 distances unless norm_search says otherwise.

        norm_search=True (vote="diagonal" only): diag_votes' norm_search, the candidate search under the normalised score. Independent
        of normalize; with both, the query rows' statistics are computed once. Refused with vote="sequence", with rerank=True and on
        a prefilter=True index; ignored with songs= (nothing is searched)."""
        vote, bin_rows, min_hits = _vote_options("locate", vote, bin_rows, min_hits, rerank, norm_search)
        if norm_search:
            self._norm_search_checks("locate")
        if normalize and rerank:
            raise ValueError("locate: normalize=True is not offered with rerank=True: the classifier's cells are probabilities and "
                             "their threshold already has a meaning")
        if normalize:
            self._need_cohort("locate")
        if rerank:
            self._check_rerank()
        elif threshold is None:
            raise ValueError("locate: threshold has no default for fingerprint scores (the reference has no such number and none has "
                             "been measured on real audio): pass one, or use rerank=True")
        n_songs, k = int(n_songs), int(k_probe)
        if n_songs < 1:
            raise ValueError(f"locate: n_songs = {n_songs} must be at least 1")
        if not 1 <= k <= ops.SEARCH_MAX_K:
            raise ValueError(f"k_probe = {k} is outside [1, {ops.SEARCH_MAX_K}]")
        if songs is not None and exclude is not None:
            raise ValueError("locate: exclude applies to the candidate search; with songs= leave the song out")
        if songs is not None and leave_out is not None:
            raise ValueError("locate: leave_out applies to the candidate search; with songs= leave the song out")
        if exclude is not None:
            self.code(exclude)
        if leave_out is not None:
            self.code(leave_out)
        fp, nodes = self._query(specs, wave, fp, nodes, rerank)
        q_stats = None
        if songs is None:
            self._check_fp(fp, "locate", device=False)
            max_q = ops.ALIGN_MAX_ROWS if rerank else self._max_q
            if fp.shape[0] > max_q:
                raise ValueError(f"locate: a query of {fp.shape[0]} rows is past the limit of {max_q}; longer inputs are "
                                 "refused, not split")
            if norm_search and fp.shape[0] and self.n_ref:        # (an empty query or index is refused below, before any launch)
                _need_cuda(fp, "locate")
                fp = fp.contiguous()
                q_stats = ops.cohort_stats(fp, self._cohort)
            songs = self._candidates(fp, nodes, k, n_songs, exclude, rerank, leave_out, vote, bin_rows, min_hits, norm_search, q_stats)
        per_song = self.align(fp, songs, threshold, min_score, top, nodes, rerank, row_hop_s=row_hop_s, row_len_s=row_len_s,
                              normalize=normalize, _q_stats=q_stats)
        flat = [(o, c, n) for c, occs in enumerate(per_song) for n, o in enumerate(occs)]
        flat.sort(key=lambda t: (-t[0].score, t[1], t[2]))
        return [t[0] for t in flat]

    @torch.no_grad()
    def paths(self, fp: torch.Tensor, occurrences: Sequence["Occurrence"], threshold: Optional[float] = None, row_hop_s=None,
              row_len_s=None, s_budget_bytes: int = 1 << 30, normalize: bool = False) -> List["AlignmentPath"]:
        """The alignment path of every occurrence, in order: which song row each query row of the occurrence was aligned to
        (AlignmentPath). occurrences: what align, locate, scan or links returned for these rows with this threshold, any selection of
        them in any order; fp: the query's rows as align / locate / scan(fp=...) took them (for a scan the whole recording's rows, since
        an occurrence's q_rows are global; for links the rows of the song that was the query). The song is Occurrence.song.

        An occurrence's path is recovered from its own box: the scores of its query rows against its song rows are recomputed by
        pair_sim (an element's bits depend on its two rows alone) and traced by align_paths, bit for bit the path of the walk that found
        it. Consecutive occurrences go in chunks whose score workspace (4 bytes a cell) stays under s_budget_bytes (one occurrence is
        always allowed): one pair_sim, one align_paths and one copy to the host per chunk.

        Refused before anything is launched: CPU rows, a missing or NaN threshold, an unknown song (KeyError), an occurrence whose rows
        leave fp or the song, an occurrence of more than ops.ALIGN_PATH_MAX rows on either side (not split). Refused afterwards
        (ValueError naming the occurrence): a box that is not an occurrence of these rows at this threshold, or whose last H differs in
        any bit from Occurrence.score; either means that the occurrences were not made from these rows with this threshold. That is
        also what happens to the occurrences of rerank=True, whose cells are the classifier's scores: their paths are not built.

        normalize=True: the occurrences were found with normalize=True (same cohort); the boxes are recomputed by pair_sim with the
        same statistics, and AlignmentPath's scores are normalised cells. Occurrences of one kind with the flag of the other fail
        the score check above."""
        if threshold is None:
            raise ValueError("paths: threshold has no default: pass the one the occurrences were found with")
        threshold = float(threshold)
        if threshold != threshold:
            raise ValueError("paths: threshold is NaN")
        timing = self._row_timing(row_hop_s, row_len_s)
        self._check_fp(fp, "paths")
        occurrences = list(occurrences)
        Lq, P = int(fp.shape[0]), len(occurrences)
        box = np.zeros((P, 5), dtype=np.int64)          # i0, rows, first ref row, columns, j0
        for n, o in enumerate(occurrences):
            if not isinstance(o, Occurrence):
                raise TypeError(f"paths: occurrences[{n}] is not an Occurrence")
            first, rows = self._song_rows[self.code(o.song)][:2]
            (i0, i1), (j0, j1) = o.q_rows, o.r_rows
            if not (0 <= i0 <= i1 < Lq and 0 <= j0 <= j1 < rows):
                raise ValueError(f"paths: occurrences[{n}] ({o.song!r}, query rows {o.q_rows}, song rows {o.r_rows}) leaves the "
                                 f"{Lq} query rows or the song's {rows} rows")
            if max(i1 - i0, j1 - j0) >= ops.ALIGN_PATH_MAX:
                raise ValueError(f"paths: occurrences[{n}] ({o.song!r}) spans {i1 - i0 + 1} x {j1 - j0 + 1} rows, past the limit of "
                                 f"{ops.ALIGN_PATH_MAX}; longer occurrences are refused, not split")
            box[n] = (i0, i1 - i0 + 1, first + j0, j1 - j0 + 1, j0)
        out: List[AlignmentPath] = []
        if P == 0:
            return out
        fp, ref, budget = fp.contiguous(), self.fingerprints, int(s_budget_bytes)
        norm = self._norm("paths", fp) if normalize else None
        lo = 0
        while lo < P:
            hi, used = lo, 0
            while hi < P and (hi == lo or used + 4 * int(box[hi, 1] * box[hi, 3]) <= budget):
                used += 4 * int(box[hi, 1] * box[hi, 3])
                hi += 1
            b = box[lo:hi]
            S, s_off, s_ld = ops.pair_sim(fp, ref, b[:, 0], b[:, 1], b[:, 2], b[:, 3], norm=norm)
            plen, poff, pi, pj, ps, end_h = ops.align_paths(S, s_off, s_ld, b[:, 1], b[:, 3], threshold, i_base=b[:, 0], j_base=b[:, 4])
            host = torch.cat([plen, end_h.view(torch.int32), pi, pj, ps.view(torch.int32)]).cpu().numpy()      # the one copy
            nb, total = hi - lo, int(pi.numel())
            plen, end_h = host[:nb], host[nb:2 * nb].view(np.float32)
            pi, pj, ps = (host[2 * nb + u * total: 2 * nb + (u + 1) * total] for u in range(3))
            ps = ps.view(np.float32)
            for n in range(nb):
                o = occurrences[lo + n]
                if plen[n] < 1 or end_h[n].tobytes() != np.float32(o.score).tobytes():
                    raise ValueError(f"paths: occurrences[{lo + n}] ({o.song!r}, query rows {o.q_rows}, song rows {o.r_rows}, score "
                                     f"{o.score!r}) is not an occurrence of these rows at threshold {threshold!r} (path_len "
                                     f"{int(plen[n])}, last H {float(end_h[n])!r})")
                a, e = int(poff[n]), int(poff[n]) + int(plen[n])
                out.append(alignment_path(o, pi[a:e], pj[a:e], ps[a:e], threshold, timing))
            lo = hi
        return out

    @staticmethod
    def _windows(Lq, k):
        """the vote windows of a query of Lq rows: (starts, W)"""
        W = min(Lq, max(1, ops.VOTE_MAX_CAND // k))
        starts = list(range(0, Lq - W + 1, W))
        if starts[-1] + W < Lq:
            starts.append(Lq - W)
        return starts, W

    @staticmethod
    def _best_songs(codes, totals):
        """song codes of some windows' top lists (-1 = none), by their best window total (descending, then by code)"""
        best = {}
        for c, total in zip(codes, totals):
            if c >= 0 and (c not in best or total > best[c]):
                best[c] = total
        return sorted(best, key=lambda c: (-best[c], c))

    def _candidates(self, fp, nodes, k, n_songs, exclude, rerank, leave_out=None, vote="sequence", bin_rows=DIAG_BIN_ROWS,
                    min_hits=DIAG_MIN_HITS, norm_search=False, q_stats=None) -> List[str]:
        """the songs of any window's top list, by their best window total (descending, then by code), at most n_songs"""
        Lq = int(fp.shape[0])
        if Lq == 0:
            raise ValueError("locate: the query has no row")
        starts, W = self._windows(Lq, k)
        codes, totals, _ = self._window_votes(fp, starts, [W] * len(starts), k, min(ops.VOTE_MAX_TOP, max(n_songs, 1)),
                                              None if exclude is None else [exclude] * len(starts),
                                              None if leave_out is None else [leave_out] * len(starts), rerank, nodes, vote, bin_rows,
                                              min_hits, norm_search, q_stats)
        order = self._best_songs(codes.reshape(-1).tolist(), totals.reshape(-1).tolist())
        return [self.names[c] for c in order[:n_songs]]

    # ------------------------------------------------------------------------------------------------ scanning a long recording
    def scanner(self, threshold: Optional[float] = None, min_score: float = 0.0, k_probe: int = 20, n_songs: int = 5, top: int = 16,
                window_rows: Optional[int] = None, songs: Optional[Sequence[str]] = None, exclude: Optional[str] = None,
                max_active: int = 64, row_hop_s=None, row_len_s=None, vote: str = "sequence", bin_rows: int = DIAG_BIN_ROWS,
                min_hits: int = DIAG_MIN_HITS, normalize: bool = False, norm_search: bool = False) -> "Scanner":
        """A Scanner over this index: a recording of any length, pushed in pieces of any sizes, is voted on and aligned in windows of
        W = window_rows or VOTE_MAX_CAND // k_probe rows (at most min(VOTE_MAX_CAND // k_probe, ALIGN_MAX_ROWS)), aligned to the global
        row index, so the result depends on the rows alone. The alignment is locate's rule, carried from window to window
        (ops.local_align_strip): a path that crosses a window boundary is one occurrence, found once. See Scanner for the active-set
        and run rules. songs=[names]: exactly these songs are aligned in every window and nothing is voted (the streaming form of
        align). exclude: a song name that never votes. threshold has no default, as in align. With long_songs a window whose active
        songs include one of more than ALIGN_MAX_COLS rows goes through local_align_panels. vote="diagonal", bin_rows, min_hits:
        locate's (the window's vote is diag_votes', so an excerpt that starts deep inside a window, or lies wholly inside one, is
        aligned in that window). normalize=True: align's; a window's rows get their cohort statistics in one launch, the
        resident rows' are cached. norm_search=True (vote="diagonal" only): locate's; a window's vote searches under the normalised
        score, and the window's statistics are the one launch normalize=True uses. Every refusal comes before any launch."""
        vote, bin_rows, min_hits = _vote_options("scanner", vote, bin_rows, min_hits, False, norm_search)
        if norm_search:
            self._norm_search_checks("scanner")
        if threshold is None:
            raise ValueError("scanner: threshold has no default for fingerprint scores (the reference has no such number and none has "
                             "been measured on real audio): pass one")
        threshold, min_score = float(threshold), float(min_score)
        if threshold != threshold or min_score != min_score:
            raise ValueError("scanner: threshold or min_score is NaN")
        n_songs, k, top, max_active = int(n_songs), int(k_probe), int(top), int(max_active)
        if n_songs < 1 or max_active < 1:
            raise ValueError(f"scanner: n_songs = {n_songs} and max_active = {max_active} must be at least 1")
        if not 1 <= k <= ops.SEARCH_MAX_K:
            raise ValueError(f"k_probe = {k} is outside [1, {ops.SEARCH_MAX_K}]")
        if not 1 <= top <= ops.ALIGN_MAX_TOP:
            raise ValueError(f"scanner: top = {top} is outside [1, {ops.ALIGN_MAX_TOP}]")
        if songs is not None and exclude is not None:
            raise ValueError("scanner: exclude applies to the vote; with songs= leave the song out")
        cap = min(max(1, ops.VOTE_MAX_CAND // k), ops.ALIGN_MAX_ROWS)
        W = cap if window_rows is None else int(window_rows)
        if W < 1:
            raise ValueError(f"scanner: window_rows = {W} must be at least 1")
        fixed = None
        if songs is not None:
            if isinstance(songs, str):
                raise TypeError("scanner: songs must be a sequence of names, not one string")
            fixed = [self.code(s) for s in songs]
            if len(set(fixed)) != len(fixed):
                raise ValueError("scanner: a song is named twice")
            for c in fixed:
                self._scan_song_ok(c)
        timing, exclude = self._row_timing(row_hop_s, row_len_s), None if exclude is None else self.code(exclude)
        if normalize:
            self._need_cohort("scanner")
        return Scanner(self, fixed, threshold, min_score, k, n_songs, top, min(W, cap), exclude, max_active, timing, vote, bin_rows,
                       min_hits, bool(normalize), bool(norm_search))

    def _scan_song_ok(self, c):
        if self._song_rows[c][1] > self._max_cols:
            raise ValueError(f"scanner: song {self.names[c]!r} has {self._song_rows[c][1]} rows, past the limit of {self._max_cols}; "
                             "longer inputs are refused, not split")

    @torch.no_grad()
    def scan(self, specs=None, wave=None, fp=None, **kw) -> List["Occurrence"]:
        """The occurrences of resident songs in a recording of any length: encodes as identify does (the whole recording first), then
        scanner(**kw).push(rows) and finish()."""
        sc = self.scanner(**kw)
        fp, _ = self._query(specs, wave, fp, None, False)
        sc.push(fp)
        return sc.finish()

    # ------------------------------------------------------------------------------------------------ the catalogue against itself
    @torch.no_grad()
    def links(self, names: Optional[Sequence[str]] = None, k_probe: int = 20, n_songs: int = 5, threshold: Optional[float] = None,
              min_score: float = 0.0, top: int = 16, block_rows: int = 1 << 16, s_budget_bytes: int = 1 << 30, row_hop_s=None,
              row_len_s=None, vote: str = "sequence", bin_rows: int = DIAG_BIN_ROWS,
              min_hits: int = DIAG_MIN_HITS, normalize: bool = False, norm_search: bool = False) -> "CatalogueLinks":
        """Which resident songs share material with which others? The self-join of the catalogue: for every named song (default: all,
        in add order) the query is the song's own resident fingerprint rows (nothing is encoded again or copied to the host), and
        occurrences[name] is what locate(fp=those rows, leave_out=name, k_probe=..., n_songs=..., threshold=..., min_score=..., top=...)
        returns, the same tuples and score bits. Both directions are reported (when A samples B, B also shares those rows with A);
        nothing is deduplicated.

        The work is batched: the songs go in blocks of at most block_rows rows (a longer song is a block of its own); a block is one
        leave-one-out search over all its rows, each row with its own song's range, one seq_scores and one song_vote over the windows
        of all its songs (locate's windows, per song), one round to the host for the candidate lists, and then every (song, candidate)
        pair through pair_sim and local_align over the resident rows in chunks whose score workspace stays under s_budget_bytes. The
        launches of a block do not grow with its number of songs.

        skipped: the songs of more than ALIGN_MAX_ROWS rows, which are not queried, and those of more than ALIGN_MAX_COLS rows, which
        are no candidates either (they are dropped from a song's candidate list before it is cut to n_songs, where locate would refuse
        the call); with long_songs both limits are ALIGN_MAX_SONG_ROWS, and a long song is queried in strips (align). threshold has no default, as in locate. There is no rerank here: the index keeps the candidates'
        [K | P] rows, not the queries' projection, so a song's rows cannot be the classifier's query side.

        vote="diagonal", bin_rows, min_hits: locate's; the block's windows go through one diag_vote instead of seq_scores + song_vote,
        and a partner sampled in the middle of a long song is a candidate by its diagonal, not by chance.

        normalize=True: locate's; both sides of every pair are resident rows, so both take the cached resident statistics.

        norm_search=True (vote="diagonal" only): locate's; a block's query rows are resident rows and take the cached resident
        statistics, so nothing is computed per block."""
        vote, bin_rows, min_hits = _vote_options("links", vote, bin_rows, min_hits, False, norm_search)
        if norm_search:
            self._norm_search_checks("links")
        if threshold is None:
            raise ValueError("links: threshold has no default for fingerprint scores (the reference has no such number and none has "
                             "been measured on real audio): pass one")
        threshold = float(threshold)
        if threshold != threshold:
            raise ValueError("links: threshold is NaN")
        n_songs, k, top, block_rows = int(n_songs), int(k_probe), int(top), int(block_rows)
        if n_songs < 1:
            raise ValueError(f"links: n_songs = {n_songs} must be at least 1")
        if not 1 <= k <= ops.SEARCH_MAX_K:
            raise ValueError(f"k_probe = {k} is outside [1, {ops.SEARCH_MAX_K}]")
        if not 1 <= top <= ops.ALIGN_MAX_TOP:
            raise ValueError(f"links: top = {top} is outside [1, {ops.ALIGN_MAX_TOP}]")
        if block_rows < 1:
            raise ValueError(f"links: block_rows = {block_rows} must be at least 1")
        if isinstance(names, str):
            raise TypeError("links: names must be a sequence of names, not one string")
        timing = self._row_timing(row_hop_s, row_len_s)
        codes = list(range(len(self.names))) if names is None else [self.code(n) for n in names]
        if len(set(codes)) != len(codes):
            raise ValueError("links: a song is named twice")
        if self.n_ref == 0:
            raise RuntimeError("SampleIndex: the index holds no song")
        rows_of = [n for _, n, _ in self._song_rows]
        too_long = {c for c, n in enumerate(rows_of) if n > self._max_cols}
        skipped = [self.names[c] for c in codes if rows_of[c] > self._max_q or c in too_long]
        query = [c for c in codes if rows_of[c] <= self._max_q and c not in too_long]
        out = {self.names[c]: [] for c in query}
        vote_top = min(ops.VOTE_MAX_TOP, max(n_songs, 1))
        norm = self._norm("links", None, resident_query=True) if normalize else None
        ref_stats = self._resident_stats("links") if norm_search else None
        lo = 0
        while lo < len(query):
            hi, used = lo, 0
            while hi < len(query) and (hi == lo or used + rows_of[query[hi]] <= block_rows):
                used += rows_of[query[hi]]
                hi += 1
            self._links_block(query[lo:hi], k, n_songs, vote_top, too_long, threshold, min_score, top, int(s_budget_bytes), timing, out,
                              vote, bin_rows, min_hits, norm, ref_stats)
            lo = hi
        return CatalogueLinks(out, skipped)

    def _links_block(self, block, k, n_songs, vote_top, too_long, threshold, min_score, top, budget, timing, out, vote="sequence",
                     bin_rows=DIAG_BIN_ROWS, min_hits=DIAG_MIN_HITS, norm=None, ref_stats=None):
        """one block of links: the songs `block` (codes) as queries; fills out[name]. ref_stats: the resident rows' statistics for a
        normalised candidate search (norm_search=True), else None."""
        first = np.asarray([self._song_rows[c][0] for c in block], dtype=np.int64)
        count = np.asarray([self._song_rows[c][1] for c in block], dtype=np.int64)
        base = np.cumsum(count) - count                           # a song's first row in the block's query table
        ref = self.fingerprints
        q_stats = None
        if (first[1:] == first[:-1] + count[:-1]).all():           # neighbours in add order: the resident rows themselves
            fp = ref[int(first[0]): int(first[-1] + count[-1])]
            if ref_stats is not None:
                q_stats = tuple(t[int(first[0]): int(first[-1] + count[-1])] for t in ref_stats)
        else:
            rows = torch.from_numpy(np.repeat(first - base, count) + np.arange(int(count.sum()))).to(self.device)
            fp = ref.index_select(0, rows)
            if ref_stats is not None:
                q_stats = tuple(t.index_select(0, rows) for t in ref_stats)
        starts, lens, owner = [], [], []
        for b, c in enumerate(block):
            s, W = self._windows(int(count[b]), k)
            starts += [int(base[b]) + v for v in s]
            lens += [W] * len(s)
            owner += [b] * len(s)
        codes, totals, _ = self._window_votes(fp, starts, lens, k, vote_top, None, [self.names[block[b]] for b in owner], False, None,
                                              vote, bin_rows, min_hits, ref_stats is not None, q_stats)
        owner = np.asarray(owner)
        pairs = []                                                # (song of the block, candidate code), a song's candidates in order
        for b in range(len(block)):
            mine = owner == b
            order = self._best_songs(codes[mine].reshape(-1).tolist(), totals[mine].reshape(-1).tolist())
            pairs += [(b, c) for c in [c for c in order if c not in too_long][:n_songs]]
        found = {b: [] for b in range(len(block))}
        occ, sc = self._align_pairs(ref, np.asarray([first[b] for b, _ in pairs], dtype=np.int64),
                                    np.asarray([count[b] for b, _ in pairs], dtype=np.int64), [c for _, c in pairs], threshold, min_score,
                                    top, budget, norm=norm)
        for p, (b, c) in enumerate(pairs):
            for n, ((i0, i1, j0, j1), s) in enumerate(zip(occ[p].tolist(), sc[p].tolist())):
                if i0 < 0:
                    break
                found[b].append((_occurrence(self.names[c], s, i0, i1, j0, j1, timing), p, n))
        for b, c in enumerate(block):                             # locate's order: by score, then candidate rank, then occurrence rank
            found[b].sort(key=lambda t: (-t[0].score, t[1], t[2]))
            out[self.names[c]] = [t[0] for t in found[b]]


class CatalogueLinks(NamedTuple):
    occurrences: dict                             # {song name: [Occurrence], as locate(fp=its rows, leave_out=name) returns them}
    skipped: List[str]                            # songs past ALIGN_MAX_ROWS / ALIGN_MAX_COLS rows (long_songs: ALIGN_MAX_SONG_ROWS): not queried, no candidates


class Scanner:
    """The state of one scan (SampleIndex.scanner). push(fp) takes (n, d) fp32 device rows, any n >= 0; finish() flushes the last,
    partial window and returns the occurrences, sorted by (-score, song code, i0, j0), in global rows of the recording.

    Per window t: one identify_pairs vote over the window (none with songs=). The active set is the songs active in window t - 1
    whose open_h > 0 (a path is still open in their carried rows), by open_h descending, then code, followed by the vote's first n_songs
    songs that are not among them, in the vote's order; what lies past max_active is closed and counted in stats["closed_at_cap"].
    Then one pair_sim and one local_align_strip for all active songs; a song that was not active in t - 1 starts fresh. A song's
    maximal stretch of consecutive active windows is a run; the rows of every run go through one align_occurrences call at finish().

    trace: one dict per window, host values: start, rows, vote_codes, vote_totals, active (codes, in order), open_h (after the strip),
    vote_hints. With vote="diagonal" the window's vote is diag_votes' (songs of at least min_hits hits in one bin), vote_totals are
    the counts, and vote_hints holds per voted song (first, last row of the recording; first, last row of the song) over the hits of
    its winning bin; with the sequence vote vote_hints is empty.
    stats: windows, strips (pairs aligned), runs, rows, closed_at_cap. runs (after finish): per run a dict with song, code, first_row,
    n_rows and the device row results row_h, row_j, row_i0, row_j0.
    With long_songs the carry pool has ALIGN_MAX_SONG_ROWS columns per slot, a window with a song of more than ALIGN_MAX_COLS rows among
    its active ones is one local_align_panels launch instead, and finish() gives align_occurrences every run's span.
    Not here: rerank cells, leave_out, songs of more than ALIGN_MAX_COLS rows (long_songs: ALIGN_MAX_SONG_ROWS), a streaming front end,
    hipGraph capture, several GPUs;
    a run is at most ops.ALIGN_OCC_MAX_ROWS rows."""

    def __init__(self, index, fixed, threshold, min_score, k, n_songs, top, W, exclude, max_active, timing, vote="sequence",
                 bin_rows=DIAG_BIN_ROWS, min_hits=DIAG_MIN_HITS, normalize=False, norm_search=False):
        self.index, self._fixed, self._theta, self._min_score = index, fixed, threshold, min_score
        self._k, self._n_songs, self._top, self.window_rows, self._exclude, self._max_active = k, n_songs, top, W, exclude, max_active
        self._timing = timing
        self._vote, self._bin_rows, self._min_hits = vote, bin_rows, min_hits
        self._normalize = normalize       # the cells are cohort-normalised: a window's rows get their statistics in one launch
        self._norm_search = norm_search   # the window's vote searches under the normalised score, on the same statistics
        self._pend = None                 # rows pushed and not yet in a window
        self._next = 0                    # global index of the first pending row
        self._active: List[int] = []      # window t - 1
        self._open = {}                   # code -> open_h after window t - 1
        self._slot = {}                   # code -> slot of the carry pool
        self._free: List[int] = []
        self._pool = None
        self._run = {}                    # code -> the open run: [first_row, parts]; a part = (rows of a window, offset, n)
        self._closed = []                 # (code, first_row, parts)
        self._done = False
        self.trace: List[dict] = []
        self.stats = {"windows": 0, "strips": 0, "runs": 0, "rows": 0, "closed_at_cap": 0}
        self.runs: List[dict] = []

    def push(self, fp: torch.Tensor) -> None:
        if self._done:
            raise RuntimeError("Scanner.push: the scan is finished")
        self.index._check_fp(fp, "Scanner.push")
        if fp.shape[0] == 0:
            return
        self._pend = fp if self._pend is None else torch.cat([self._pend, fp])
        W = self.window_rows
        while self._pend.shape[0] >= W:
            self._window(self._pend[:W])
            self._pend = self._pend[W:]
        if self._pend.shape[0] == 0:
            self._pend = None
        else:
            self._pend = self._pend.clone()          # the caller's tensor is not kept

    def _carry_pool(self):
        if self._pool is None:
            slots = max(self._max_active, len(self._fixed or ()))
            self._pool, _ = ops.align_carry([self.index._max_cols] * slots, self.index.device, long_songs=self.index.long_songs)
            self._free = list(range(slots - 1, -1, -1))
        return self._pool

    def _close(self, c):
        first, parts = self._run.pop(c)
        self._closed.append((c, first, parts))
        self._free.append(self._slot.pop(c))
        self._open.pop(c, None)

    @torch.no_grad()
    def _window(self, rows):
        idx, start, n = self.index, self._next, int(rows.shape[0])
        rows = rows.contiguous()
        vote_codes, vote_totals, vote_hints = [], [], []
        q_stats = None                    # the window's statistics, once for the vote's search and for the cells
        if self._fixed is not None:
            want = list(self._fixed)
        else:
            if self._norm_search:
                q_stats = ops.cohort_stats(rows, idx._need_cohort("scanner"))
            codes, totals, hints = idx._window_votes(rows, [0], [n], self._k, min(ops.VOTE_MAX_TOP, self._n_songs),
                                                     None if self._exclude is None else [idx.names[self._exclude]], None, False, None,
                                                     self._vote, self._bin_rows, self._min_hits, self._norm_search, q_stats)
            codes, totals = codes[0], totals[0]
            m = int((codes >= 0).sum())                              # the diagonal vote's songs below min_hits are a tail: counts descend
            vote_codes, vote_totals = codes[:m].tolist(), totals[:m].tolist()
            if hints is not None:
                vote_hints = [(start + int(h[0]), start + int(h[1]), int(h[2]) - idx._song_rows[c][0], int(h[3]) - idx._song_rows[c][0])
                              for c, h in zip(vote_codes, hints[0][:m])]
            cont = sorted((c for c in self._active if self._open[c] > 0), key=lambda c: (-self._open[c], c))
            want = cont + [c for c in vote_codes[: self._n_songs] if c not in cont]
            self.stats["closed_at_cap"] += max(0, len(want) - self._max_active)
            want = want[: self._max_active]
            for c in want:
                idx._scan_song_ok(c)
        pool = self._carry_pool()
        for c in [c for c in self._active if c not in want]:
            self._close(c)
        fresh = []
        for c in want:
            fresh.append(0 if c in self._run else 1)
            if c not in self._run:
                self._run[c] = [start, []]
                self._slot[c] = self._free.pop()
                self.stats["runs"] += 1
        open_h = []
        if want:
            P = len(want)
            x_start = np.asarray([idx._song_rows[c][0] for c in want], dtype=np.int64)
            x_len = np.asarray([idx._song_rows[c][1] for c in want], dtype=np.int64)
            q_len = np.full(P, n, dtype=np.int64)
            panels = bool((x_len > ops.ALIGN_MAX_COLS).any())              # a long song among them: every pair in one panels launch
            norm = idx._norm("scanner", rows, q_stats=q_stats) if self._normalize else None
            S, s_off, s_ld = ops.pair_sim(rows, idx.fingerprints, np.zeros(P, np.int64), q_len, x_start, x_len, long_songs=panels,
                                          norm=norm)
            carry_off = np.asarray([self._slot[c] for c in want], dtype=np.int64) * (2 * idx._max_cols)
            strip = ops.local_align_panels if panels else ops.local_align_strip
            *res, row_off, oh = strip(S, s_off, s_ld, q_len, x_len, self._theta, np.full(P, start, np.int64), fresh, pool, carry_off)
            open_h = oh.cpu().numpy().astype(np.float64).tolist()
            for p, c in enumerate(want):
                self._run[c][1].append((res, int(row_off[p]), n))
                self._open[c] = open_h[p]
        self._active = want
        self._next = start + n
        self.trace.append({"start": start, "rows": n, "vote_codes": vote_codes, "vote_totals": vote_totals, "active": list(want),
                           "open_h": open_h, "vote_hints": vote_hints})
        self.stats["windows"] += 1
        self.stats["strips"] += len(want)
        self.stats["rows"] += n

    @torch.no_grad()
    def finish(self) -> List["Occurrence"]:
        if self._done:
            raise RuntimeError("Scanner.finish: the scan is finished")
        if self._pend is not None:
            self._window(self._pend)
            self._pend = None
        for c in list(self._active):
            self._close(c)
        self._active, self._done = [], True
        runs = [r for r in self._closed if r[2]]
        out = []
        if runs:
            flat = [torch.cat([res[u][off:off + n] for _, _, parts in runs for res, off, n in parts]) for u in range(4)]
            n_rows = np.asarray([sum(n for _, _, n in parts) for _, _, parts in runs], dtype=np.int64)
            row_off = np.cumsum(n_rows) - n_rows
            first = np.asarray([f for _, f, _ in runs], dtype=np.int64)
            span = None
            if self.index.long_songs:
                span = np.asarray([max(2 * (self.index._song_rows[c][1] - 1), 0) for c, _, _ in runs], dtype=np.int64)
            occ, sc, _ = ops.align_occurrences(*flat, row_off, n_rows, first, self._min_score, self._top, span=span)
            occ, sc = occ.cpu().numpy(), sc.cpu().numpy()
            for r, (c, f, _) in enumerate(runs):
                lo, hi = int(row_off[r]), int(row_off[r] + n_rows[r])
                self.runs.append({"song": self.index.names[c], "code": c, "first_row": int(f), "n_rows": int(n_rows[r]),
                                  "row_h": flat[0][lo:hi], "row_j": flat[1][lo:hi], "row_i0": flat[2][lo:hi], "row_j0": flat[3][lo:hi]})
                for (i0, i1, j0, j1), s in zip(occ[r].tolist(), sc[r].tolist()):
                    if i0 < 0:
                        break
                    out.append((c, _occurrence(self.index.names[c], s, i0, i1, j0, j1, self._timing)))
        self._closed = []
        out.sort(key=lambda t: (-t[1].score, t[0], t[1].q_rows[0], t[1].r_rows[0]))
        return [o for _, o in out]


class Occurrence(NamedTuple):
    song: str
    score: float
    q_rows: Tuple[int, int]                       # (first, last) row, inclusive, of the query
    r_rows: Tuple[int, int]                       # the same of the song
    q_time: Optional[Tuple[float, float]]         # seconds, when the row timing is known
    r_time: Optional[Tuple[float, float]]
    stretch: float                                # (j1 - j0) / (i1 - i0): song rows per query row; nan for a one-row occurrence


def _occurrence(song, score, i0, i1, j0, j1, timing) -> Occurrence:
    qt = rt = None
    if timing is not None:
        hop, length = timing
        qt, rt = (i0 * hop, i1 * hop + length), (j0 * hop, j1 * hop + length)
    return Occurrence(song, float(score), (int(i0), int(i1)), (int(j0), int(j1)), qt, rt,
                      (j1 - j0) / (i1 - i0) if i1 > i0 else float("nan"))


class AlignmentPath(NamedTuple):
    """The path of an occurrence (SampleIndex.paths): cell t aligns query row q_rows[t] with song row r_rows[t]; both arrays rise
    strictly, by (1, 1), (1, 2) or (2, 1) a step, from the occurrence's first rows to its last. The statistics need no calibrated
    score; no cut-off on them is set anywhere."""
    occurrence: "Occurrence"
    q_rows: np.ndarray                            # (cells,) int32, global query rows
    r_rows: np.ndarray                            # (cells,) int32, song rows
    scores: np.ndarray                            # (cells,) float32: S at the cell
    steps: Tuple[int, int, int]                   # the steps taken: (1, 1), (1, 2), (2, 1); cells - 1 in all
    passing: int                                  # the cells whose own fp32 S - threshold is positive
    slope: Optional[float]                        # fp64 least-squares line, song row = slope * query row + intercept: song rows per query
    intercept: Optional[float]                    # row, the tempo estimate over the whole path; None for a path of one cell
    rms_rows: Optional[float]                     # root mean square of the path's deviation from that line, in song rows
    q_time: Optional[np.ndarray]                  # (cells,) float64: the start of each row in seconds, when the row timing is known
    r_time: Optional[np.ndarray]

    def song_row(self, q_row):
        """the song row (fractional) aligned with a query row: piecewise linear along the path, clamped to its ends"""
        return np.interp(q_row, self.q_rows, self.r_rows)

    def song_time(self, t):
        """the second of the song aligned with second t of the query, as song_row; needs the row timing"""
        if self.q_time is None:
            raise ValueError("AlignmentPath.song_time: the row timing is not known (row_hop_s / row_len_s, or an index with a front end)")
        return np.interp(t, self.q_time, self.r_time)


def alignment_path(occurrence, q_rows, r_rows, scores, threshold, timing=None) -> AlignmentPath:
    """an AlignmentPath from a path's cells in forward order; timing: (row hop, row length) in seconds or None"""
    q = np.ascontiguousarray(q_rows, dtype=np.int32)
    r = np.ascontiguousarray(r_rows, dtype=np.int32)
    s = np.ascontiguousarray(scores, dtype=np.float32)
    if not (q.ndim == 1 and q.size >= 1 and q.shape == r.shape == s.shape):
        raise ValueError("alignment_path: q_rows, r_rows and scores must be three equal, non-empty one-dimensional arrays")
    di, dj = np.diff(q.astype(np.int64)), np.diff(r.astype(np.int64))
    steps = tuple(int(((di == a) & (dj == b)).sum()) for a, b in ((1, 1), (1, 2), (2, 1)))
    if sum(steps) != q.size - 1:
        raise ValueError("alignment_path: the cells do not follow one another by (1, 1), (1, 2) or (2, 1)")
    passing = int(((s - np.float32(threshold)).astype(np.float32) > 0).sum())
    slope = intercept = rms = None
    if q.size > 1:
        x, y = q.astype(np.float64), r.astype(np.float64)
        xm, ym = x.mean(), y.mean()
        slope = float(((x - xm) * (y - ym)).sum() / ((x - xm) ** 2).sum())
        intercept = float(ym - slope * xm)
        rms = float(np.sqrt(((y - (slope * x + intercept)) ** 2).mean()))
    qt = rt = None
    if timing is not None:
        qt, rt = q.astype(np.float64) * timing[0], r.astype(np.float64) * timing[0]
    return AlignmentPath(occurrence, q, r, s, steps, passing, slope, intercept, rms, qt, rt)


def interval_recall(found, truth, min_cover: float = 0.5):
    """Segment-wise evaluation of located occurrences against annotated ones (the query_time_annotations / target_time_annotations of
    sample100-ext, as plain lists): found, truth = lists of (start, end) seconds. A truth interval counts as found when the union of the
    found intervals covers at least min_cover of it (a truth interval of zero length: when a found interval contains it). Returns
    (recall, covered_seconds, found_seconds_outside_truth): recall = found truth intervals / truth intervals (nan without truth),
    covered_seconds = the length of union(found) inside union(truth), the last = the length of union(found) outside it."""
    def union(iv):
        iv = sorted((float(a), float(b)) for a, b in iv)
        out = []
        for a, b in iv:
            if b < a:
                raise ValueError(f"interval_recall: an interval ends before it starts: ({a}, {b})")
            if out and a <= out[-1][1]:
                out[-1][1] = max(out[-1][1], b)
            else:
                out.append([a, b])
        return out

    def overlap(a, b, iv):
        return sum(max(0.0, min(b, d) - max(a, c)) for c, d in iv)

    fu, tu = union(found), union(truth)
    hits = 0
    for a, b in truth:
        a, b = float(a), float(b)
        if b > a:
            hits += overlap(a, b, fu) >= float(min_cover) * (b - a)
        else:
            hits += any(c <= a <= d for c, d in fu)
    covered = sum(overlap(a, b, fu) for a, b in tu)
    total_found = sum(b - a for a, b in fu)
    recall = hits / len(truth) if len(truth) else float("nan")
    return recall, covered, total_found - covered


def rejection_stats(real_scores, dummy_scores, threshold: float = 0.5):
    """ablation.py:111-139 without the plot: (auroc, true_rejects, false_accepts). AUROC of real (label 1) against dummy (label 0)
    scores by ranks with ties averaged (Mann-Whitney U / (n1 n0), what sklearn's roc_auc_score computes); true_rejects = dummies
    below the threshold, false_accepts = dummies at or above it."""
    real = np.asarray(real_scores, dtype=np.float64).reshape(-1)
    dummy = np.asarray(dummy_scores, dtype=np.float64).reshape(-1)
    if real.size == 0 or dummy.size == 0:
        raise ValueError("rejection_stats: both score lists must be non-empty")
    if np.isnan(real).any() or np.isnan(dummy).any():
        raise ValueError("rejection_stats: a score is NaN")
    scores = np.concatenate([real, dummy])
    order = np.argsort(scores, kind="stable")
    sorted_scores = scores[order]
    first = np.flatnonzero(np.r_[True, sorted_scores[1:] != sorted_scores[:-1]])
    count = np.diff(np.r_[first, scores.size])
    avg_rank = np.repeat(first + (count + 1) / 2.0, count)          # 1-based ranks, ties averaged
    rank = np.empty(scores.size)
    rank[order] = avg_rank
    u = rank[: real.size].sum() - real.size * (real.size + 1) / 2.0
    auroc = float(u / (real.size * dummy.size))
    return auroc, int((dummy < threshold).sum()), int((dummy >= threshold).sum())
