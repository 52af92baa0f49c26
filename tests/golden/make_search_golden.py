"""Generator of tests/golden/search_l2.npz: the reference's own exact-mode evaluation (eval.py eval_faiss, index_type='l2') on
rule-made fingerprint databases.

    python tests/golden/make_search_golden.py --reference-repo <checkout of chymaera96/NeuralSampleID> [--seed 0]

The reference needs FAISS, which this stack does not have: a stand-in `faiss` module is put into sys.modules whose IndexFlatL2
is exact fp64 brute force with a stable argsort (ties -> smaller id). eval.py is loaded by path and eval_faiss runs on a temporary
copy of the databases (it extends dummy_db.mm in place) from a temporary working directory holding data/gt_dict.json.

Inputs are made by rule from a seed (make_inputs): unit-norm d = 128 rows; ref songs of random length; queries are noisy slices of
ref songs at graded noise, plus a few with no true song; query ids differ from the ref song names. The generator asserts two
margins and moves to the next seed until both hold, so that an fp32 implementation must reproduce the fixture exactly:
  - every query row's fp64 distances: k-th and (k+1)-th differ by >= 1e-4, and neighbouring ranks inside the top k by >= 1e-6
    (a row that misses them gets its noise drawn again, by rule);
  - in every (test, sl), the song scores that decide a top-1, top-3 or top-10 outcome differ by >= 1e-4.
The fixture stores the seed and parameters, a digest of the generated inputs, the stand-in's I for every query row and the
reference's hit_rates, raw_score and test_ids. Tests regenerate the inputs with load_golden_inputs() and never read the reference."""
import argparse
import hashlib
import importlib.util
import json
import os
import shutil
import sys
import tempfile
import types
from collections import defaultdict

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "search_l2.npz")
PARAMS = {"d": 128, "n_songs": 30, "seg_min": 12, "seg_max": 48, "n_dummy": 2000, "n_queries": 20, "n_false": 3,
          "len_max": 22, "noise": [0.1, 0.3, 0.5, 0.7, 0.9, 1.1], "k_probe": 20, "test_seq_len": "1 3 5 9 11 19"}
KTH_GAP, RANK_GAP, SCORE_GAP = 1e-4, 1e-6, 1e-4


def _unit(a):
    return a / np.linalg.norm(a, axis=1, keepdims=True)


def _dist(q, x):
    q, x = q.astype(np.float64), x.astype(np.float64)
    return (q * q).sum(1)[:, None] + (x * x).sum(1)[None, :] - 2.0 * q @ x.T


def _row_ok(dist_row, k):
    s = np.sort(dist_row)[: k + 1]
    return s[k] - s[k - 1] >= KTH_GAP and (np.diff(s[:k]) >= RANK_GAP).all()


def make_inputs(seed, p=PARAMS):
    """the rule: numpy PCG64 from `seed`; returns dict of float32 arrays ref / dummy / query, lookups and gt"""
    rng = np.random.Generator(np.random.PCG64(seed))
    d, k = p["d"], p["k_probe"]
    lens = rng.integers(p["seg_min"], p["seg_max"] + 1, size=p["n_songs"])
    ref = _unit(rng.standard_normal((int(lens.sum()), d))).astype(np.float32)
    names = [f"song{i:03d}" for i in range(p["n_songs"])]
    ref_lookup = [n for n, c in zip(names, lens) for _ in range(int(c))]
    song_start = np.concatenate([[0], np.cumsum(lens)[:-1]])
    dummy = _unit(rng.standard_normal((p["n_dummy"], d))).astype(np.float32)
    xb = np.concatenate([dummy, ref])
    gt = {n: [] for n in names}
    rows, query_lookup = [], []
    for qi in range(p["n_queries"]):
        qid = f"q{qi:03d}"
        L = int(rng.integers(1, p["len_max"] + 1))
        true = qi < p["n_queries"] - p["n_false"]
        if true:
            song = int(rng.integers(p["n_songs"]))
            L = min(L, int(lens[song]))
            s0 = int(song_start[song] + rng.integers(0, int(lens[song]) - L + 1))
            sigma = p["noise"][qi % len(p["noise"])]
            gt[names[song]].append(qid)
        for i in range(L):
            for _ in range(200):                    # redraw the row (by rule) until its fp64 ranking has the margins
                if true:
                    r = ref[s0 + i] + sigma * rng.standard_normal(d) / np.sqrt(d)
                else:
                    r = rng.standard_normal(d)
                r = _unit(r[None, :]).astype(np.float32)
                if _row_ok(_dist(r, xb)[0], k):
                    break
            else:
                raise RuntimeError("no row with the distance margins in 200 draws")
            rows.append(r[0])
            query_lookup.append(f"{qid}_{qi}")
    return {"ref": ref, "dummy": dummy, "query": np.stack(rows), "ref_lookup": ref_lookup, "query_lookup": query_lookup, "gt": gt}


def digest(inp):
    h = hashlib.sha256()
    for key in ("ref", "dummy", "query"):
        h.update(np.ascontiguousarray(inp[key]).tobytes())
    h.update(json.dumps([inp["ref_lookup"], inp["query_lookup"], inp["gt"]], sort_keys=True).encode())
    return h.hexdigest()


def write_inputs(inp, emb_dir):
    """the three databases in the reference's format (fpdb.write_fp_db: byte-identical to test_fp.py's writer)"""
    from neuralsampleid_amd.fpdb import write_fp_db
    write_fp_db(emb_dir, "ref_db", inp["ref"], inp["ref_lookup"])
    write_fp_db(emb_dir, "dummy_db", inp["dummy"], ["dummy"] * inp["dummy"].shape[0])
    write_fp_db(emb_dir, "query_db", inp["query"], inp["query_lookup"])


def load_golden_inputs():
    """(the fixture, its inputs regenerated by rule); asserts the rule still reproduces the fixture's inputs"""
    with np.load(FIXTURE) as f:
        z = {key: f[key] for key in f.files}
    params = json.loads(bytes(z["params"]).decode())
    inp = make_inputs(int(z["seed"]), params)
    got = digest(inp)
    assert got == str(z["digest"]), ("the rule no longer reproduces the golden's inputs (numpy's PCG64 / normal stream changed?): "
                                     "regenerate with tests/golden/make_search_golden.py")
    return z, inp


def sequence_scores(I, query, xb, starts, lens, sl_all, k):
    """fp64 candidate scores in make_pairs order (eval.py:325-331)"""
    from neuralsampleid_amd.search import make_pairs
    _, _, ps, pl = make_pairs(starts, lens, sl_all)
    out = np.full((ps.size, int(np.max(pl)) * k if ps.size else 0), np.nan)
    q64, x64 = query.astype(np.float64), xb.astype(np.float64)
    for p, (s, L) in enumerate(zip(ps, pl)):
        for j in range(L * k):
            cid = I[s + j // k, j % k]
            if cid < 0:
                continue
            n = min(L, xb.shape[0] - cid)
            out[p, j] = np.mean(np.sum(q64[s:s + n] * x64[cid:cid + n], axis=1))
    return out


def score_margins_ok(I, inp, p):
    """in every (test, sl): the song scores at the top-1 / top-3 / top-10 boundaries differ by >= SCORE_GAP"""
    from neuralsampleid_amd.search import extract_test_ids, parse_seq_len
    k, nd = p["k_probe"], inp["dummy"].shape[0]
    xb = np.concatenate([inp["dummy"], inp["ref"]]).astype(np.float64)
    q = inp["query"].astype(np.float64)
    starts, lens = extract_test_ids(inp["query_lookup"])
    for s, L in zip(starts, lens):
        qid = inp["query_lookup"][s].split("_")[0]
        for sl in parse_seq_len(p["test_seq_len"]):
            if sl > L:
                continue
            hist = defaultdict(float)
            for cid in I[s:s + sl][I[s:s + sl] >= 0].ravel():
                if cid < nd or inp["ref_lookup"][cid - nd] == qid:
                    continue
                n = min(sl, xb.shape[0] - cid)
                hist[inp["ref_lookup"][cid - nd]] += np.mean(np.sum(q[s:s + n] * xb[cid:cid + n], axis=1))
            v = sorted(hist.values(), reverse=True)
            for b in (1, 3, 10):
                if len(v) > b and v[b - 1] - v[b] < SCORE_GAP:
                    return False
    return True


class _FlatL2:
    """stand-in for faiss.IndexFlatL2: exact fp64 brute force, stable argsort (ties -> smaller id)"""

    def __init__(self, d):
        self.d, self.xb, self.nprobe = d, np.zeros((0, d), np.float32), 1

    @property
    def ntotal(self):
        return self.xb.shape[0]

    def train(self, x):
        pass

    def add(self, x):
        self.xb = np.concatenate([self.xb, np.asarray(x, np.float32)])

    def search(self, q, k):
        dist = _dist(np.asarray(q), self.xb)
        I = np.argsort(dist, axis=1, kind="stable")[:, :k]
        D = np.take_along_axis(dist, I, 1).astype(np.float32)
        if k > self.ntotal:
            pad = k - self.ntotal
            I = np.concatenate([I, -np.ones((I.shape[0], pad), np.int64)], 1)
            D = np.concatenate([D, np.full((D.shape[0], pad), np.inf, np.float32)], 1)
        return D, I.astype(np.int64)


def _fake_faiss():
    m = types.ModuleType("faiss")
    m.IndexFlatL2 = _FlatL2
    return m


def run_reference(reference_repo, inp, p):
    sys.modules["faiss"] = _fake_faiss()
    spec = importlib.util.spec_from_file_location("_ref_eval", os.path.join(reference_repo, "eval.py"))
    ev = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ev)
    cwd = os.getcwd()
    with tempfile.TemporaryDirectory() as tmp:
        emb = os.path.join(tmp, "emb")
        write_inputs(inp, emb)
        os.makedirs(os.path.join(tmp, "data"))
        with open(os.path.join(tmp, "data", "gt_dict.json"), "w") as f:
            json.dump(inp["gt"], f)
        try:
            os.chdir(tmp)
            ev.eval_faiss(emb, index_type="l2", nogpu=True, test_seq_len=p["test_seq_len"], k_probe=p["k_probe"])
        finally:
            os.chdir(cwd)
        return {n: np.load(os.path.join(emb, n + ".npy")) for n in ("hit_rates", "raw_score", "test_ids")}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference-repo", required=True)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    root = os.path.dirname(os.path.dirname(HERE))
    if root not in sys.path:
        sys.path.insert(0, root)
    p = PARAMS
    for seed in range(a.seed, a.seed + 1000):
        inp = make_inputs(seed, p)
        idx = _FlatL2(p["d"])
        idx.add(inp["dummy"])
        idx.add(inp["ref"])
        _, I = idx.search(inp["query"], p["k_probe"])
        if score_margins_ok(I, inp, p):
            break
        print(f"seed {seed}: a song-score margin below {SCORE_GAP}, next seed")
    else:
        raise RuntimeError("no seed with the margins")
    out = run_reference(a.reference_repo, inp, p)
    np.savez_compressed(FIXTURE, seed=np.int64(seed), params=np.frombuffer(json.dumps(p).encode(), np.uint8),
                        digest=np.array(digest(inp)), I=I.astype(np.int32), **out)
    print(f"seed {seed}: {inp['query'].shape[0]} query rows, {inp['ref'].shape[0]} ref rows; hit rates\n{out['hit_rates']}\n"
          f"-> {FIXTURE} ({os.path.getsize(FIXTURE)} bytes)")


if __name__ == "__main__":
    main()
