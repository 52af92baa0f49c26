"""Classifier re-rank evaluation on the GPU: hit rates and MAP@k (csrc/rerank.hip through classifier.CrossAttentionClassifier).

Reference: eval_hr.py:41-163 `eval_faiss_clf` and eval_map.py:14-177 `eval_faiss_map_clf` / `calculate_map`, as test_fp.py:419-461
calls them. Both search the fingerprint index for candidates, re-score every candidate segment with the stage-2 classifier on the
encoder's pre-projection node matrices (ref_nmatrix/{song}.npy, query_nmatrix.npy / query_full_nmatrix.npy) and vote per song.

Here the candidates come from FlatL2Index over dummy ++ ref (the reference with index_type='l2'); every query row is searched once.
Each ref song's node matrices are loaded once, and only if one of its segments is a candidate; every query and candidate segment is
projected once; the pairs of all tests are scored in one blocked kernel call. The song-level votes and the MAP are host functions
(vote_hit_rates_clf, vote_map_clf, calculate_map) that take I and per-test score matrices, so they run without a GPU.

Differences from the reference, all deliberate:
  * the MAP's candidates are exact: the reference's eval_faiss_map_clf is always called with index_type='ivfpq' (test_fp.py:454),
    a trained approximate index whose candidates depend on FAISS's training;
  * input files are never written (the reference's load_memmap_data opens the databases 'r+' and rewrites NaNs in place);
  * a ref song missing from gt counts as no hit / not relevant where the hit-rate evaluation raises KeyError;
  * skipped candidates (missing node-matrix file, segment past its rows) are counted and reported once, not printed one by one.

    python -m neuralsampleid_amd.rerank --emb-dir D --gt gt_dict.json --clf-ckpt clf.pth [--dummy-dir D] [--map] [--k-probe N]
"""
import argparse
import os
import warnings
from collections import defaultdict
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from . import ops
from .search import _load_db, _load_gt, extract_test_ids, format_hit_rates, parse_seq_len

OUT_BLOCK = 1 << 26           # scores per clf_pair_scores call at most (256 MB of output)
PROJ_BLOCK = 4096             # segments per projection call


# ------------------------------------------------------------------------------------------------ host side
def calculate_map(ground_truth, predictions, k=10):
    """eval_map.py:14-40: mean over the predictions dict of AP@k = mean of precision@i at the hits within the first k (not divided
    by the number of relevant items; 0 without a hit); a song missing from ground_truth is not relevant"""
    average_precisions = []
    for q_id, retrieved_list in predictions.items():
        num_relevant = 0
        precision_values = []
        for i, retrieved_id in enumerate(retrieved_list[:k]):
            if q_id in ground_truth.get(retrieved_id, []):
                num_relevant += 1
                precision_values.append(num_relevant / (i + 1))
        average_precisions.append(np.mean(precision_values) if precision_values else 0)
    return np.mean(average_precisions) if average_precisions else 0


def ref_run_starts(ref_lookup: Sequence[str]) -> np.ndarray:
    """per ref row, the first row of its run of equal names (eval_hr.py:113 ref_song_starts[ref_song_starts <= ref_id].max())"""
    starts, lens = extract_test_ids(ref_lookup)
    return np.repeat(starts, lens)


class _Walk:
    """the candidate rules shared by both votes: cid -> (song, segment) or None, counting the skips"""

    def __init__(self, ref_lookup, n_dummy, ref_rows):
        self.ref_lookup, self.n_dummy, self.ref_rows = ref_lookup, int(n_dummy), ref_rows
        self.run_start = ref_run_starts(ref_lookup) if len(ref_lookup) else np.zeros(0, np.int64)
        self.missing = self.out_of_bounds = 0

    def segment(self, cid: int, q_id: str):
        if cid < 0 or cid < self.n_dummy or cid - self.n_dummy >= len(self.ref_lookup):
            return None
        ref_id = cid - self.n_dummy
        song = self.ref_lookup[ref_id]
        if song == q_id:
            return None
        rows = self.ref_rows.get(song)
        if rows is None:
            self.missing += 1
            return None
        seg = ref_id - int(self.run_start[ref_id])
        if seg >= rows:
            self.out_of_bounds += 1
            return None
        return song, seg


def _column(cand_ids: np.ndarray, cid: int) -> int:
    j = int(np.searchsorted(cand_ids, cid))
    if j >= cand_ids.size or cand_ids[j] != cid:
        raise ValueError(f"candidate {cid} has no column in its test's score matrix")
    return j


def candidate_ids(I_rows: np.ndarray, q_id: str, walk: "_Walk") -> np.ndarray:
    """the ascending unique ids of I_rows that pass the candidate rules (the columns of a test's score matrix)"""
    ids = np.unique(I_rows[I_rows >= 0])
    keep = [int(c) for c in ids.tolist() if walk.segment(int(c), q_id) is not None]
    return np.asarray(keep, dtype=np.int64)


def vote_hit_rates_clf(I, test_scores, query_lookup, ref_lookup, n_dummy, gt, ref_rows, test_seq_len='1 3 5 9 11 19'):
    """The song-level vote of eval_hr.py:85-156 on the host.

    I: (query rows, k) ids over dummy ++ ref; test_scores[t] = (cand_ids ascending, S (rows, len(cand_ids))): the classifier scores
    of test t's query segments (the first rows of query_nmatrix[q_id]) against its candidate ids; ref_rows: {song: rows of
    ref_nmatrix/{song}.npy} (a song without a file is absent). Per (test, sl) the candidates of I[start : start + sl] are walked
    row-major; ids < 0, dummies and the query's own song are skipped, and so are candidates without a node-matrix file or with a
    segment index past its rows. Score = max over the first sl rows of the candidate's column; it is added to its song when >= 0.5
    (a repeated candidate adds again). Songs rank by descending sum, ties in first-appearance order. Returns (hit_rates (3, L) float64
    percent, raw_score (tests, 3 L) int64, test_ids int64, (missing, out_of_bounds) skip counts)."""
    I = np.asarray(I)
    sl_all = parse_seq_len(test_seq_len)
    starts, lens = extract_test_ids(query_lookup)
    if len(test_scores) != starts.size:
        raise ValueError(f"vote_hit_rates_clf: {len(test_scores)} score matrices for {starts.size} tests")
    walk = _Walk(ref_lookup, n_dummy, ref_rows)
    n_test, n_sl = starts.size, sl_all.size
    top = np.zeros((3, n_test, n_sl), dtype=int)
    for ti, (s0, L) in enumerate(zip(starts.tolist(), lens.tolist())):
        q_id = query_lookup[s0].split("_")[0]
        cand_ids, S = test_scores[ti]
        cand_ids, S = np.asarray(cand_ids), np.asarray(S)
        for si, sl in enumerate(sl_all.tolist()):
            if sl > L:
                continue
            hist = defaultdict(float)
            rows = I[s0:s0 + sl]
            for cid in rows[rows >= 0].tolist():
                seg = walk.segment(int(cid), q_id)
                if seg is None:
                    continue
                score = float(S[:sl, _column(cand_ids, int(cid))].max())
                if score >= 0.5:
                    hist[seg[0]] += score
            pred = sorted(hist, key=hist.get, reverse=True)
            for m, lim in enumerate((1, 3, 10)):
                top[m, ti, si] = int(any(q_id in gt.get(p, ()) for p in pred[:lim]))
    valid = sl_all[None, :] <= lens[:, None]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)          # a length no test reaches: NaN, as the reference's nanmean gives
        hit_rates = np.stack([100 * np.nanmean(np.where(valid, top[m], np.nan), axis=0) for m in range(3)], axis=0)
    raw_score = np.concatenate([top[0], top[1], top[2]], axis=1)
    return hit_rates, raw_score, starts, (walk.missing, walk.out_of_bounds)


def vote_map_clf(I, test_scores, query_lookup, ref_lookup, n_dummy, ref_rows):
    """The vote of eval_map.py:112-165 on the host: per test the candidates are np.unique(I[start : start + len][I >= 0]) in
    ascending order (frequencies ignored), with the rules of vote_hit_rates_clf; score = max over ALL rows of the column, weight =
    score if score > 0.5 else 0, and the song enters the vote even at 0 (ties rank in insertion order). A repeated q_id overwrites
    its earlier prediction and keeps its dict position. Returns (predictions {q_id: [songs]}, (missing, out_of_bounds))."""
    I = np.asarray(I)
    starts, lens = extract_test_ids(query_lookup)
    if len(test_scores) != starts.size:
        raise ValueError(f"vote_map_clf: {len(test_scores)} score matrices for {starts.size} tests")
    walk = _Walk(ref_lookup, n_dummy, ref_rows)
    predictions = {}
    for ti, (s0, L) in enumerate(zip(starts.tolist(), lens.tolist())):
        q_id = query_lookup[s0].split("_")[0]
        cand_ids, S = test_scores[ti]
        cand_ids, S = np.asarray(cand_ids), np.asarray(S)
        rows = I[s0:s0 + L]
        hist = defaultdict(int)
        for cid in np.unique(rows[rows >= 0]).tolist():
            seg = walk.segment(int(cid), q_id)
            if seg is None:
                continue
            score = float(S[:, _column(cand_ids, int(cid))].max())
            hist[seg[0]] += score if score > 0.5 else 0
        predictions[q_id] = sorted(hist, key=hist.get, reverse=True)
    return predictions, (walk.missing, walk.out_of_bounds)


# ------------------------------------------------------------------------------------------------ GPU side
def _ref_rows(ref_nmatrix_dir: str, songs) -> Dict[str, int]:
    """{song: rows of its node-matrix file} for the songs that have one (the header only: no data is read)"""
    out = {}
    for song in songs:
        path = os.path.join(ref_nmatrix_dir, f"{song}.npy")
        if os.path.exists(path):
            out[song] = int(np.load(path, mmap_mode="r").shape[0])
    return out


def _check_nm(a: np.ndarray, what: str, C: int = ops.CLF_C) -> int:
    if a.ndim != 3 or a.shape[1] != C:
        raise ValueError(f"{what}: node matrices must be (segments, {C}, N) for a classifier of in_dim {C}, got {a.shape}: the "
                         "classifier checkpoint and the node matrices come from encoders of different sizes")
    return int(a.shape[2])


def checkpoint_in_dim(state) -> int:
    """in_dim of a CrossAttentionClassifier state_dict: the columns of attn.in_proj_weight (3 in_dim x in_dim)"""
    w = state.get("attn.in_proj_weight") if hasattr(state, "get") else None
    if w is None or len(w.shape) != 2 or w.shape[0] != 3 * w.shape[1]:
        raise ValueError("the classifier checkpoint has no packed attn.in_proj_weight of shape (3 in_dim, in_dim): not a "
                         "CrossAttentionClassifier state_dict")
    return int(w.shape[1])


def checkpoint_num_nodes(state):
    """(num_nodes, pos_embed) of a CrossAttentionClassifier state_dict: the rows of its positional_embedding buffer (1, num_nodes,
    in_dim); a checkpoint written with pos_embed=False has no such key and gives (the constructor's default 100, False)"""
    pe = state.get("positional_embedding") if hasattr(state, "get") else None
    if pe is None:
        return 100, False
    if len(pe.shape) != 3 or pe.shape[0] != 1 or pe.shape[1] < 1:
        raise ValueError(f"the classifier checkpoint's positional_embedding has shape {tuple(pe.shape)}, not (1, num_nodes, in_dim)")
    return int(pe.shape[1]), True


def _project(fn, arrays: List[np.ndarray], device) -> torch.Tensor:
    """concatenated projections of a list of (S_i, C, N) arrays, PROJ_BLOCK segments per call"""
    parts, buf, nbuf = [], [], 0
    for a in arrays + [None]:
        if a is not None:
            buf.append(a)
            nbuf += a.shape[0]
        if nbuf and (a is None or nbuf >= PROJ_BLOCK):
            x = torch.from_numpy(np.ascontiguousarray(np.concatenate(buf), dtype=np.float32)).to(device)
            parts.append(fn(x))
            buf, nbuf = [], 0
    if not parts:
        return None
    return torch.cat(parts) if len(parts) > 1 else parts[0]


def score_tests(classifier, tests, query_nm: Dict[str, np.ndarray], ref_nmatrix_dir: str, ref_lookup, n_dummy, device="cuda"):
    """tests: list of (q_id, query rows to use, candidate ids ascending). Projects every needed query segment and candidate segment
    once (a ref song's file is loaded once, and only if it has a candidate) and scores all tests' (rows x candidates) blocks.
    Returns the list of (cand_ids, S (rows, candidates) float32 numpy)."""
    run_start = ref_run_starts(ref_lookup) if len(ref_lookup) else np.zeros(0, np.int64)
    C = int(classifier.attn.embed_dim)
    # query segments: one block per q_id, as many rows as its tests need
    q_rows = {}
    for q_id, rows, _ in tests:
        q_rows[q_id] = max(q_rows.get(q_id, 0), rows)
    q_off, q_arrays, N = {}, [], None
    for q_id, rows in q_rows.items():
        a = query_nm[q_id]
        n = _check_nm(a, f"query node matrices of {q_id!r}", C)
        if N is not None and n != N:
            raise ValueError(f"node matrices disagree on N ({N} vs {n})")
        N = n
        q_off[q_id] = sum(x.shape[0] for x in q_arrays)
        q_arrays.append(np.asarray(a[:rows]))
    # candidate segments: unique over all tests, grouped by song
    all_c = np.unique(np.concatenate([c for _, _, c in tests])) if tests else np.zeros(0, np.int64)
    c_index = {int(c): i for i, c in enumerate(all_c.tolist())}
    c_arrays = []
    by_song = defaultdict(list)
    for c in all_c.tolist():
        ref_id = c - n_dummy
        by_song[ref_lookup[ref_id]].append((c, ref_id - int(run_start[ref_id])))
    seg_rows = [None] * all_c.size
    for song, items in by_song.items():
        a = np.load(os.path.join(ref_nmatrix_dir, f"{song}.npy"))       # once per song with a candidate
        n = _check_nm(a, f"ref_nmatrix/{song}.npy", C)
        if N is not None and n != N:
            raise ValueError(f"node matrices disagree on N ({N} vs {n})")
        N = n
        for c, seg in items:
            seg_rows[c_index[c]] = a[seg]
    if all_c.size:
        c_arrays = [np.stack(seg_rows)]
    results = [(c, np.zeros((rows, c.size), np.float32)) for _, rows, c in tests]
    if not tests or all_c.size == 0 or not any(rows and c.size for _, rows, c in tests):
        return results
    with torch.no_grad():
        q = _project(classifier.project_queries, q_arrays, device)
        kp = _project(classifier.project_candidates, c_arrays, device)
        # groups = tests with pairs, in blocks of at most OUT_BLOCK scores per call
        order = [t for t, (_, rows, c) in enumerate(tests) if rows and c.size]
        a = 0
        while a < len(order):
            b, n = a, 0
            while b < len(order) and (b == a or n + tests[order[b]][1] * tests[order[b]][2].size <= OUT_BLOCK):
                n += tests[order[b]][1] * tests[order[b]][2].size
                b += 1
            blk = order[a:b]
            cidx = [np.asarray([c_index[int(c)] for c in tests[t][2].tolist()], np.int64) for t in blk]
            coff = np.concatenate([[0], np.cumsum([x.size for x in cidx])[:-1]])
            out, off = classifier.score_blocks(q, kp, N, [q_off[tests[t][0]] for t in blk], [tests[t][1] for t in blk],
                                               np.concatenate(cidx), coff, [x.size for x in cidx])
            host = out.cpu().numpy()
            for t, o, ci in zip(blk, off.tolist(), cidx):
                rows = tests[t][1]
                results[t] = (tests[t][2], host[o:o + rows * ci.size].reshape(rows, ci.size))
            a = b
    return results


def _load_query_nm(path):
    nm = np.load(path, allow_pickle=True).item()
    if not isinstance(nm, dict):
        raise ValueError(f"{path}: expected np.save of a dict {{song: (S, C, N) node matrices}}")
    return nm


def _query_nm(nm, q_id, path):
    if q_id not in nm:
        raise KeyError(f"no query node matrices for {q_id!r} in {path}")
    if np.asarray(nm[q_id]).shape[0] == 0:
        raise ValueError(f"the query node matrices of {q_id!r} in {path} have no segments")
    return nm[q_id]


def _report(skips, what):
    missing, oob = skips
    if missing or oob:
        print(f"{what}: skipped {missing} candidates without a ref_nmatrix file and {oob} with a segment past their file's rows")


def eval_hit_rates_clf(emb_dir: str, classifier, gt, emb_dummy_dir: Optional[str] = None, test_seq_len='1 3 5 9 11 19',
                       k_probe: int = 5, save: bool = True, device="cuda"):
    """eval_hr.py eval_faiss_clf(emb_dir, classifier, emb_dummy_dir, index_type='l2', test_seq_len=..., k_probe=...) on the GPU.

    Reads query_db / ref_db (emb_dir), dummy_db (emb_dummy_dir, default emb_dir), query_nmatrix.npy and ref_nmatrix/; gt: {ref song:
    [query ids]} or its JSON path. Returns hit_rates (3, len(test_seq_len)) in percent; with save writes hit_rates_clf.npy,
    raw_score_clf.npy and test_ids_clf.npy into emb_dir. Input files are never modified."""
    gt = _load_gt(gt)
    sl = parse_seq_len(test_seq_len)
    k_probe = int(k_probe)
    if not 1 <= k_probe <= ops.SEARCH_MAX_K:
        raise ValueError(f"k_probe = {k_probe} is outside [1, {ops.SEARCH_MAX_K}]")
    classifier.eval()
    emb_dummy_dir = emb_dir if emb_dummy_dir is None else emb_dummy_dir
    index, qt, query_lookup, ref_lookup, n_dummy = _load_db(emb_dir, emb_dummy_dir, "query_db", device)
    nm_path = os.path.join(emb_dir, "query_nmatrix.npy")
    query_nm = _load_query_nm(nm_path)
    ref_dir = os.path.join(emb_dir, "ref_nmatrix")
    _, I = index.search(qt, k_probe)
    I = I.cpu().numpy()
    ref_rows = _ref_rows(ref_dir, sorted(set(ref_lookup)))
    walk = _Walk(ref_lookup, n_dummy, ref_rows)
    starts, lens = extract_test_ids(query_lookup)
    tests = []
    for s0, L in zip(starts.tolist(), lens.tolist()):
        q_id = query_lookup[s0].split("_")[0]
        nm_rows = np.asarray(_query_nm(query_nm, q_id, nm_path)).shape[0]
        msl = int(sl[sl <= L].max()) if (sl <= L).any() else 0
        if msl == 0:
            tests.append((q_id, 0, np.zeros(0, np.int64)))
            continue
        nq = min(msl, nm_rows)
        tests.append((q_id, nq, candidate_ids(I[s0:s0 + msl], q_id, walk)))
    scores = score_tests(classifier, tests, query_nm, ref_dir, ref_lookup, n_dummy, device)
    hit_rates, raw_score, test_ids, skips = vote_hit_rates_clf(I, scores, query_lookup, ref_lookup, n_dummy, gt, ref_rows, sl)
    _report(skips, "eval_hit_rates_clf")
    if save:
        np.save(os.path.join(emb_dir, "hit_rates_clf.npy"), hit_rates)
        np.save(os.path.join(emb_dir, "raw_score_clf.npy"), raw_score)
        np.save(os.path.join(emb_dir, "test_ids_clf.npy"), test_ids)
    return hit_rates


def eval_map_clf(emb_dir: str, classifier, gt, emb_dummy_dir: Optional[str] = None, k_probe: int = 3, k_map: int = 20,
                 save: bool = True, device="cuda"):
    """eval_map.py eval_faiss_map_clf(emb_dir, classifier, emb_dummy_dir, k_probe=..., k_map=...) on the GPU, with EXACT candidates
    (FlatL2Index; the reference always runs it on a trained IVF-PQ index).

    Reads query_full_db (emb_dir, lookup of plain names), ref_db, dummy_db, query_full_nmatrix.npy and ref_nmatrix/. Returns
    (map_score, k_map); with save writes predictions.npy (np.save of the dict) and map_score.npy into emb_dir. Input files are never
    modified."""
    gt = _load_gt(gt)
    k_probe = int(k_probe)
    if not 1 <= k_probe <= ops.SEARCH_MAX_K:
        raise ValueError(f"k_probe = {k_probe} is outside [1, {ops.SEARCH_MAX_K}]")
    classifier.eval()
    emb_dummy_dir = emb_dir if emb_dummy_dir is None else emb_dummy_dir
    index, qt, query_lookup, ref_lookup, n_dummy = _load_db(emb_dir, emb_dummy_dir, "query_full_db", device)
    nm_path = os.path.join(emb_dir, "query_full_nmatrix.npy")
    query_nm = _load_query_nm(nm_path)
    ref_dir = os.path.join(emb_dir, "ref_nmatrix")
    _, I = index.search(qt, k_probe)
    I = I.cpu().numpy()
    ref_rows = _ref_rows(ref_dir, sorted(set(ref_lookup)))
    walk = _Walk(ref_lookup, n_dummy, ref_rows)
    starts, lens = extract_test_ids(query_lookup)
    tests = []
    for s0, L in zip(starts.tolist(), lens.tolist()):
        q_id = query_lookup[s0].split("_")[0]
        nq = np.asarray(_query_nm(query_nm, q_id, nm_path)).shape[0]
        tests.append((q_id, nq, candidate_ids(I[s0:s0 + L], q_id, walk)))
    scores = score_tests(classifier, tests, query_nm, ref_dir, ref_lookup, n_dummy, device)
    predictions, skips = vote_map_clf(I, scores, query_lookup, ref_lookup, n_dummy, ref_rows)
    _report(skips, "eval_map_clf")
    map_score = calculate_map(gt, predictions, k=k_map)
    if save:
        np.save(os.path.join(emb_dir, "predictions.npy"), predictions)
        np.save(os.path.join(emb_dir, "map_score.npy"), map_score)
    return map_score, k_map


def main(argv=None) -> None:
    ap = argparse.ArgumentParser(prog="python -m neuralsampleid_amd.rerank", description=__doc__.split("\n\n")[0])
    ap.add_argument("--emb-dir", required=True, help="fingerprint DBs, node matrices (query_nmatrix.npy, ref_nmatrix/)")
    ap.add_argument("--gt", required=True, help="JSON {ref song: [query ids]} (the reference's data/gt_dict.json)")
    ap.add_argument("--clf-ckpt", required=True, help="CrossAttentionClassifier state_dict (downstream.py's clf_*.pth)")
    ap.add_argument("--dummy-dir", default=None, help="directory of dummy_db (default: --emb-dir)")
    ap.add_argument("--map", action="store_true", help="also MAP@20 over query_full_db / query_full_nmatrix.npy")
    ap.add_argument("--k-probe", type=int, default=None, help="candidates per query row (default: 5 for hit rates, 3 for MAP)")
    ap.add_argument("--test-seq-len", default="1 3 5 9 11 19")
    ap.add_argument("--no-save", action="store_true", help="do not write the result files")
    a = ap.parse_args(argv)
    from .classifier import CrossAttentionClassifier
    state = torch.load(a.clf_ckpt, map_location="cuda")
    in_dim = checkpoint_in_dim(state)
    if in_dim not in ops.CLF_WIDTHS:
        ap.error(f"--clf-ckpt: a classifier of in_dim {in_dim}; the re-rank covers in_dim {', '.join(map(str, ops.CLF_WIDTHS))}")
    num_nodes, pos_embed = checkpoint_num_nodes(state)
    clf = CrossAttentionClassifier(in_dim=in_dim, num_nodes=num_nodes, pos_embed=pos_embed).cuda()
    clf.load_state_dict(state)
    clf.eval()
    hr = eval_hit_rates_clf(a.emb_dir, clf, a.gt, a.dummy_dir, a.test_seq_len, a.k_probe or 5, save=not a.no_save)
    print(format_hit_rates(hr, a.test_seq_len))
    if a.map:
        m, k = eval_map_clf(a.emb_dir, clf, a.gt, a.dummy_dir, k_probe=a.k_probe or 3, save=not a.no_save)
        print(f"MAP@{k}: {m:.4f}")


if __name__ == "__main__":
    main()
