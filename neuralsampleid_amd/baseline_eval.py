"""Evaluation of the ResNet-IBN baseline on the GPU: exact search over its 2048-d fingerprints and the baseline's own song vote.

Reference: baseline/eval_hr.py:195-371 `eval_faiss` and baseline/eval_map.py:75-181 `eval_faiss_with_map` (baseline/run_eval.py calls
both). They share eval.py's databases and search but not its vote: a candidate's score is the FAISS distance itself (the maximum
over the rows of the slice that returned it), candidates are walked in np.unique (ascending id) order, and songs are ranked by
DESCENDING summed distance. Written from the reference's behaviour, odd as that ranking is; `FlatL2Index` (the wide kernel of
csrc/search.hip at d = 2048) stands in for the FAISS index. As in search.py, every query row is searched once, a song missing from
gt counts as no hit, and no input file is modified (the reference extends dummy_db.mm in place).

    python -m neuralsampleid_amd.baseline_eval --emb-dir DIR --gt gt_dict.json [--dummy-dir DIR] [--k-probe 20]
                                               [--test-seq-len "1 3 5"] [--map] [--no-save]
"""
import argparse
import os
import warnings
from typing import Dict, List, Optional, Sequence, Tuple, Union

import numpy as np

from . import ops
from .rerank import calculate_map
from .search import _load_db, _load_gt, extract_test_ids, format_hit_rates, parse_seq_len

MAP_MIN_ROWS = 10               # eval_map.py:129: a test of this many rows or fewer is not scored


def vote_baseline(I, D, rows, q_id: str, ref_lookup: Sequence[str], n_dummy: int) -> List[str]:
    """The song vote of eval_hr.py:305-338 / eval_map.py:134-169 for one query slice: the songs in rank order.

    I, D: (query rows, k) ids over dummy ++ ref (-1 = none) and their distances; rows: the slice (a slice object or row indices).
    The candidates are the unique ids >= 0 of I[rows], ascending; a candidate's score is the maximum of its D over the slice. Ids
    below n_dummy and songs named like q_id are skipped; every song sums its candidates' scores in that order, in fp32 (the
    reference adds np.float32 scalars). Songs are ranked by descending sum, ties in first-appearance order (Python's stable
    sorted(reverse=True))."""
    Ir = np.asarray(I)[rows]
    Dr = np.asarray(D, dtype=np.float32)[rows]
    valid = Ir >= 0
    cand, inv = np.unique(Ir[valid], return_inverse=True)
    score = np.full(cand.size, -np.inf, dtype=np.float32)
    np.maximum.at(score, inv.reshape(-1), Dr[valid])
    hist: Dict[str, np.float32] = {}
    for cid, sc in zip(cand.tolist(), score):
        if cid < n_dummy:
            continue
        match = ref_lookup[cid - n_dummy]
        if match == q_id:
            continue
        hist[match] = np.float32(hist.get(match, np.float32(0.0)) + sc)
    return sorted(hist, key=hist.get, reverse=True)


def _check_ID(I, D, query_lookup, what):
    I, D = np.asarray(I), np.asarray(D)
    if I.ndim != 2 or I.shape != D.shape or I.shape[0] != len(query_lookup):
        raise ValueError(f"{what}: I and D must both be ({len(query_lookup)}, k), one row per query segment, got {I.shape} and {D.shape}")
    return I, D


def hit_rates_baseline(I, D, query_lookup: Sequence[str], ref_lookup: Sequence[str], n_dummy: int, gt: Dict[str, Sequence[str]],
                       test_seq_len='1 3 5 9 11 19') -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """eval_hr.py:283-368 on the host from one search of all query rows: per (test, length) the vote of rows [start, start + length);
    top-1/3/10 = the query id is in gt[song] for one of the first 1 / 3 / 10 songs. Returns (hit_rates (3, len(test_seq_len))
    float64 in percent, raw_score (tests, 3 len(test_seq_len)) int, test_ids = the tests' start rows)."""
    sl = parse_seq_len(test_seq_len)
    starts, lens = extract_test_ids(query_lookup)
    I, D = _check_ID(I, D, query_lookup, "hit_rates_baseline")
    if len(ref_lookup) == 0:
        raise ValueError("hit_rates_baseline: the ref lookup table is empty")
    n_dummy = int(n_dummy)
    top = np.zeros((3, starts.size, sl.size), dtype=np.int_)
    for ti, (s0, L) in enumerate(zip(starts.tolist(), lens.tolist())):
        q_id = query_lookup[s0].split("_")[0]
        for si, n in enumerate(sl[sl <= L].tolist()):              # eval_hr.py:293-295: si counts the lengths that fit
            pred = vote_baseline(I, D, slice(s0, s0 + n), q_id, ref_lookup, n_dummy)
            for m, lim in enumerate((1, 3, 10)):
                top[m, ti, si] = int(any(q_id in gt.get(p, ()) for p in pred[:lim]))
    valid = sl[None, :] <= lens[:, None]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)          # a length no test reaches: NaN, as the reference's nanmean gives
        hit_rates = np.stack([100.0 * np.nanmean(np.where(valid, top[m], np.nan), axis=0) for m in range(3)], axis=0)
    return hit_rates, np.concatenate((top[0], top[1], top[2]), axis=1), starts


def predictions_baseline(I, D, query_lookup: Sequence[str], ref_lookup: Sequence[str], n_dummy: int) -> Dict[str, List[str]]:
    """eval_map.py:121-170: {query id: songs in rank order}, one slice per test over all its rows; a test of MAP_MIN_ROWS rows or
    fewer is skipped, and a repeated query id overwrites its earlier entry"""
    starts, lens = extract_test_ids(query_lookup)
    I, D = _check_ID(I, D, query_lookup, "predictions_baseline")
    if len(ref_lookup) == 0:
        raise ValueError("predictions_baseline: the ref lookup table is empty")
    predictions = {}
    for s0, L in zip(starts.tolist(), lens.tolist()):
        if L <= MAP_MIN_ROWS:
            continue
        q_id = query_lookup[s0].split("_")[0]
        predictions[q_id] = vote_baseline(I, D, slice(s0, s0 + L), q_id, ref_lookup, int(n_dummy))
    return predictions


def _k_probe(k_probe) -> int:
    k_probe = int(k_probe)
    if not 1 <= k_probe <= ops.SEARCH_MAX_K:
        raise ValueError(f"k_probe = {k_probe} is outside [1, {ops.SEARCH_MAX_K}]")
    return k_probe


def _search_all(emb_dir, emb_dummy_dir, query_name, k_probe, device):
    emb_dummy_dir = emb_dir if emb_dummy_dir is None else emb_dummy_dir
    index, qt, query_lookup, ref_lookup, n_dummy = _load_db(emb_dir, emb_dummy_dir, query_name, device)
    D, I = index.search(qt, k_probe)
    return I.cpu().numpy(), D.cpu().numpy(), query_lookup, ref_lookup, n_dummy


def eval_hit_rates_baseline(emb_dir: str, gt: Union[str, Dict[str, Sequence[str]]], emb_dummy_dir: Optional[str] = None,
                            test_seq_len='1 3 5 9 11 19', k_probe: int = 20, save: bool = True, device="cuda") -> np.ndarray:
    """baseline/eval_hr.py eval_faiss(emb_dir, emb_dummy_dir, index_type='l2', test_seq_len=..., k_probe=...) on the GPU.

    Reads {query,ref}_db from emb_dir and dummy_db from emb_dummy_dir (default emb_dir) in fpdb's format, NaN -> 0 on the copies;
    gt: {ref song: [query ids]} or its JSON path. Returns hit_rates (3, len(test_seq_len)): top-1/3/10 in percent per query
    length; with save writes hit_rates.npy, raw_score.npy and test_ids.npy into emb_dir as the reference does."""
    gt = _load_gt(gt)
    sl = parse_seq_len(test_seq_len)
    I, D, query_lookup, ref_lookup, n_dummy = _search_all(emb_dir, emb_dummy_dir, "query_db", _k_probe(k_probe), device)
    hit_rates, raw_score, test_ids = hit_rates_baseline(I, D, query_lookup, ref_lookup, n_dummy, gt, sl)
    if save:
        np.save(os.path.join(emb_dir, "hit_rates.npy"), hit_rates)
        np.save(os.path.join(emb_dir, "raw_score.npy"), raw_score)
        np.save(os.path.join(emb_dir, "test_ids.npy"), test_ids)
    return hit_rates


def eval_map_baseline(emb_dir: str, gt: Union[str, Dict[str, Sequence[str]]], emb_dummy_dir: Optional[str] = None, k_probe: int = 20,
                      k_map: int = 20, save: bool = True, device="cuda"):
    """baseline/eval_map.py eval_faiss_with_map(emb_dir, emb_dummy_dir, index_type='l2', k_probe=..., k_map=...) on the GPU.

    Reads query_full_db (emb_dir), ref_db and dummy_db. Returns (map_score, k_map); with save writes predictions.npy (np.save of
    the dict) and map_score.npy into emb_dir."""
    gt = _load_gt(gt)
    I, D, query_lookup, ref_lookup, n_dummy = _search_all(emb_dir, emb_dummy_dir, "query_full_db", _k_probe(k_probe), device)
    predictions = predictions_baseline(I, D, query_lookup, ref_lookup, n_dummy)
    map_score = calculate_map(gt, predictions, k=k_map)
    if save:
        np.save(os.path.join(emb_dir, "predictions.npy"), predictions)
        np.save(os.path.join(emb_dir, "map_score.npy"), map_score)
    return map_score, k_map


def main(argv=None) -> None:
    ap = argparse.ArgumentParser(prog="python -m neuralsampleid_amd.baseline_eval", description=__doc__.split("\n\n")[0])
    ap.add_argument("--emb-dir", required=True, help="directory with query_db / ref_db (and dummy_db, query_full_db) in fpdb's format")
    ap.add_argument("--gt", required=True, help="JSON {ref song: [query ids]} (the reference's data/gt_dict.json)")
    ap.add_argument("--dummy-dir", default=None, help="directory of dummy_db (default: --emb-dir)")
    ap.add_argument("--k-probe", type=int, default=20)
    ap.add_argument("--test-seq-len", default="1 3 5 9 11 19")
    ap.add_argument("--map", action="store_true", help="also MAP@20 over query_full_db")
    ap.add_argument("--no-save", action="store_true", help="do not write the result files")
    a = ap.parse_args(argv)
    hr = eval_hit_rates_baseline(a.emb_dir, a.gt, a.dummy_dir, a.test_seq_len, a.k_probe, save=not a.no_save)
    print(format_hit_rates(hr, a.test_seq_len))
    if a.map:
        m, k = eval_map_baseline(a.emb_dir, a.gt, a.dummy_dir, k_probe=a.k_probe, save=not a.no_save)
        print(f"MAP@{k}: {m:.4f}")


if __name__ == "__main__":
    main()
