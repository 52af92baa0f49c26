"""GPU: the ResNet-IBN baseline's evaluation (neuralsampleid_amd/baseline_eval.py over the wide search kernel) against the golden
made by the reference's own baseline/eval_hr.py and baseline/eval_map.py (tests/golden/make_baseline_eval_golden.py), and end to end
from the baseline model's fingerprint extraction."""
import hashlib
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _file_digests(d):
    return {f: hashlib.sha256(open(os.path.join(d, f), "rb").read()).hexdigest() for f in sorted(os.listdir(d))}


def test_baseline_eval_matches_reference_golden(tmp_path):
    from make_baseline_eval_golden import load_golden_inputs, write_inputs
    from neuralsampleid_amd.baseline_eval import eval_hit_rates_baseline, eval_map_baseline
    from neuralsampleid_amd.search import FlatL2Index
    z, inp = load_golden_inputs()
    params = json.loads(bytes(z["params"]).decode())
    assert inp["query"].shape[1] == 2048
    emb = str(tmp_path / "emb")
    write_inputs(inp, emb)
    gt_path = str(tmp_path / "gt_dict.json")
    with open(gt_path, "w") as f:
        json.dump(inp["gt"], f)
    before = _file_digests(emb)

    hr = eval_hit_rates_baseline(emb, gt_path, test_seq_len=params["test_seq_len"], k_probe=params["k_probe"])
    after = _file_digests(emb)
    assert set(after) - set(before) == {"hit_rates.npy", "raw_score.npy", "test_ids.npy"}
    np.testing.assert_array_equal(hr, z["hit_rates"])
    for name in ("hit_rates", "raw_score", "test_ids"):
        got = np.load(os.path.join(emb, name + ".npy"))
        assert got.dtype == z[name].dtype and got.shape == z[name].shape, name
        np.testing.assert_array_equal(got, z[name])

    map_score, k_map = eval_map_baseline(emb, gt_path, k_probe=params["k_probe"], k_map=params["k_map"])
    after = _file_digests(emb)
    for f, h in before.items():
        assert after[f] == h, f"{f} was modified"
    assert set(after) - set(before) == {"hit_rates.npy", "raw_score.npy", "test_ids.npy", "predictions.npy", "map_score.npy"}
    want = json.loads(str(z["predictions"]))
    assert k_map == params["k_map"] and abs(map_score - float(z["map_score"])) <= 1e-12
    assert abs(float(np.load(os.path.join(emb, "map_score.npy"))) - float(z["map_score"])) <= 1e-12
    pred = np.load(os.path.join(emb, "predictions.npy"), allow_pickle=True).item()
    assert pred == want and list(pred) == list(want)

    idx = FlatL2Index(2048, DEV)
    idx.add(inp["dummy"])
    idx.add(inp["ref"])
    _, I = idx.search(inp["query"], params["k_probe"])
    np.testing.assert_array_equal(I, z["I"].astype(np.int64))


def test_end_to_end_extraction_search(tmp_path):
    """ref DB from the baseline model's extraction of synthetic segments, query DBs from a subset of them under query names: with one
    probe per row every query row votes only for the song of its nearest row (itself), so top-1 = 100 % whatever the reference's
    descending-distance ranking would do with more"""
    from synth import synth_state
    from neuralsampleid_amd import functional as F_
    from neuralsampleid_amd import fpdb, ops
    from neuralsampleid_amd.baseline_eval import eval_hit_rates_baseline
    from neuralsampleid_amd.encoder.resnet_ibn import ResNetIBN
    from neuralsampleid_amd.search import eval_hit_rates
    from neuralsampleid_amd.simclr.triplet import BaselineModel
    F_.set_activation_dtype(torch.float32)      # process-wide switches other tests move
    ops.set_gemm_precision("fp32")
    model = BaselineModel({"arch": "resnet-ibn", "n_frames": 216}, ResNetIBN())
    sd = synth_state(model.state_dict())
    sd["encoder.global_pool.p"] = torch.full((1,), 2.5)
    model.load_state_dict(sd)
    model = model.to(DEV).eval()
    g = torch.Generator().manual_seed(11)
    x = (torch.randn(24, 84, 216, generator=g).abs() * 2).to(DEV)
    songs = [(f"song{i}", x[4 * i:4 * i + 4]) for i in range(6)]
    emb = str(tmp_path / "emb")
    assert fpdb.build_fp_db(model, songs, emb, "ref_db", batch=8) == (24, 2048)
    fpdb.build_fp_db(model, songs[:1], emb, "dummy_db", batch=8)
    queries = [(f"q{i}", x[4 * i + 1:4 * i + 3]) for i in (1, 3, 4)]
    fpdb.build_fp_db(model, queries, emb, "query_db", query_style=True, batch=8)
    gt = {f"song{i}": ([f"q{i}"] if i in (1, 3, 4) else []) for i in range(6)}
    ops.launch_counters(reset=True)
    hr = eval_hit_rates_baseline(emb, gt, test_seq_len="1 2", k_probe=1, save=False)
    assert ops.launch_counters()["flat_l2_topk_wide"] == 1
    assert hr.shape == (3, 2) and hr[0, 0] == 100.0 and hr[0, 1] == 100.0, hr
    # the shared loader and seq_scores at d = 2048: GraFP's evaluation reads the same databases
    hr2 = eval_hit_rates(emb, gt, test_seq_len="1 2", k_probe=1, save=False)
    assert hr2.shape == (3, 2) and hr2[0, 0] == 100.0 and hr2[0, 1] == 100.0, hr2
