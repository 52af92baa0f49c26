"""Generator of tests/golden/clf_train.npz: three steps of the reference's own classifier training loop (downstream.py:97-140 train,
with mine_hard_negatives) on rule-made features, on the CPU.

    python tests/golden/make_clf_train_golden.py --reference-repo <checkout of chymaera96/NeuralSampleID> [--seed 0]

downstream.py is loaded by path with DGL, tensorboard and the training modules stubbed in sys.modules (make_rerank_golden). Its train()
runs unchanged with a list loader of 3 batches, an identity augment, a stub frozen model, rule-made classifier weights,
torch.optim.Adam(lr=cfg['clf_lr']) and GradScaler(). On the CPU GradScaler disables itself (scale / step / update become a plain
backward and optimizer.step()); the repository's GPU test runs its scaler=None path against this golden.

The stub model: peak_extractor is the identity, encoder(p, return_pre_proj=True) returns the batch itself (the loader yields node
matrices), and model(x_i, x_j) returns the rule-made normalised projections of the current step. Everything else is recorded through
hooks only, changing no line of the reference: the dropout masks (output / input of fc[2]), the classifier's inputs (from which the
mined indices are recovered exactly: the node matrices are distinct) and scores (forward hooks), step-0 gradients (an optimiser step
pre-hook) and the final parameters.

The rule (make_case) draws from numpy PCG64 and moves to the next seed until these margins hold, so that an fp32 implementation must
reproduce the golden: every adjacent gap among the first k + 2 similarities of a row is >= 1e-4; every fc.0 pre-activation is >= 1e-4
away from 0; at least one candidate segment serves two or more pairs of a step. Only the rule's outputs are stored; large tensors as
per-row sums, per-column sums, their L2 norms and sampled elements (tests/golden/clf_train.npz, well under 1 MB)."""
import argparse
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "clf_train.npz")
PARAMS = {"B": 8, "C": 512, "N": 32, "num_nodes": 32, "d": 128, "k": 3, "steps": 3, "clf_lr": 1e-4, "p_drop": 0.3, "samples": 1024}
SIM_GAP, PRE_GAP = 1e-4, 1e-4
PARAM_NAMES = ["attn.in_proj_weight", "attn.in_proj_bias", "attn.out_proj.weight", "attn.out_proj.bias", "fc.0.weight", "fc.0.bias",
               "fc.3.weight", "fc.3.bias"]


def make_case(seed, p=PARAMS):
    """the rule: per step node matrices (B, C, N) of both views and normalised projections (B, d) of both views (z_j near z_i, so
    that rank 1 is often the positive view)"""
    rng = np.random.Generator(np.random.PCG64(seed))
    B, C, N, d = p["B"], p["C"], p["N"], p["d"]
    steps = []
    for _ in range(p["steps"]):
        ni = rng.standard_normal((B, C, N)).astype(np.float32)
        nj = (ni + 0.5 * rng.standard_normal((B, C, N))).astype(np.float32)
        zi = rng.standard_normal((B, d))
        zj = zi + 0.6 * rng.standard_normal((B, d))
        zi /= np.linalg.norm(zi, axis=1, keepdims=True)
        zj /= np.linalg.norm(zj, axis=1, keepdims=True)
        steps.append({"nodes_i": ni, "nodes_j": nj, "z_i": zi.astype(np.float32), "z_j": zj.astype(np.float32)})
    return steps


def classifier_state(seed, p=PARAMS):
    """the rule for the classifier's initial weights: a state_dict of float32 torch tensors in the reference's layout"""
    import torch
    rng = np.random.Generator(np.random.PCG64(seed + 104729))
    C, nn_, hid = p["C"], p["num_nodes"], 128
    n = lambda *s, scale: torch.from_numpy((rng.standard_normal(s) * scale).astype(np.float32))
    return {"positional_embedding": n(1, nn_, C, scale=0.5),
            "attn.in_proj_weight": n(3 * C, C, scale=C ** -0.5), "attn.in_proj_bias": n(3 * C, scale=0.1),
            "attn.out_proj.weight": n(C, C, scale=C ** -0.5), "attn.out_proj.bias": n(C, scale=0.1),
            "fc.0.weight": n(hid, C, scale=2.0 * C ** -0.5), "fc.0.bias": n(hid, scale=0.1),
            "fc.3.weight": n(1, hid, scale=2.0 * hid ** -0.5), "fc.3.bias": n(1, scale=0.1)}


def sample_index(seed, shape, p=PARAMS):
    """flat indices of the sampled elements of a tensor (all of it when it is small)"""
    n = int(np.prod(shape))
    if n <= p["samples"]:
        return np.arange(n)
    return np.sort(np.random.Generator(np.random.PCG64(seed + n)).choice(n, p["samples"], replace=False))


def digest(steps, state):
    h = hashlib.sha256()
    for st in steps:
        for key in sorted(st):
            h.update(np.ascontiguousarray(st[key]).tobytes())
    for key in sorted(state):
        h.update(state[key].numpy().tobytes())
    return h.hexdigest()


def compact(prefix, t, idx):
    """per-row sums, per-column sums (2-D), the L2 norm and sampled elements of a tensor"""
    a = np.asarray(t, dtype=np.float64)
    m = a.reshape(a.shape[0], -1) if a.ndim > 1 else a.reshape(1, -1)
    return {prefix + "/rows": m.sum(1), prefix + "/cols": m.sum(0), prefix + "/l2": np.array([np.linalg.norm(a)]),
            prefix + "/samples": a.reshape(-1)[idx]}


def load_golden_inputs():
    """(the fixture, the per-step features regenerated by rule, the rule classifier's initial state_dict)"""
    with np.load(FIXTURE) as f:
        z = {key: f[key] for key in f.files}
    params = json.loads(bytes(z["params"]).decode())
    steps = make_case(int(z["seed"]), params)
    state = classifier_state(int(z["seed"]), params)
    assert digest(steps, state) == str(z["digest"]), ("the rule no longer reproduces the golden's inputs: regenerate with "
                                                      "tests/golden/make_clf_train_golden.py")
    return z, params, steps, state


def run_reference(reference_repo, steps, state, p):
    import torch
    from make_rerank_golden import _fake_modules, _load
    sys.modules.update(_fake_modules())
    ds = _load(os.path.join(reference_repo, "downstream.py"), "_ref_downstream")
    torch.manual_seed(0)                            # the dropout masks: recorded, whatever they are
    clf = ds.CrossAttentionClassifier(in_dim=p["C"], num_nodes=p["num_nodes"])
    clf.load_state_dict(state, strict=True)

    class StubModel(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.step = 0
            self.peak_extractor = lambda x: x

        def encoder(self, x, return_pre_proj=False):
            return x, None

        def forward(self, x_i, x_j):
            st = steps[self.step]
            self.step += 1
            return None, None, torch.from_numpy(st["z_i"]), torch.from_numpy(st["z_j"])

    rec = {"fc2_in": [], "fc2_out": [], "fc0_out": [], "clf_in": [], "scores": [], "grads": None}
    def fc2_hook(m, i, o):
        rec["fc2_in"].append(i[0].detach().clone())
        rec["fc2_out"].append(o.detach().clone())

    def fc0_hook(m, i, o):
        rec["fc0_out"].append(o.detach().clone())

    def clf_hook(m, i, o):
        rec["clf_in"].append((i[0].detach().clone(), i[1].detach().clone()))
        rec["scores"].append(o.detach().clone())
    clf.fc[2].register_forward_hook(fc2_hook)
    clf.fc[0].register_forward_hook(fc0_hook)
    clf.register_forward_hook(clf_hook)
    opt = torch.optim.Adam(clf.parameters(), lr=p["clf_lr"])

    def pre_hook(o, args, kwargs):
        if rec["grads"] is None:
            rec["grads"] = {n: q.grad.detach().clone() for n, q in clf.named_parameters()}
    opt.register_step_pre_hook(pre_hook)
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")              # GradScaler on a machine without CUDA: disabled, with a warning
        scaler = ds.GradScaler()
    loader = [(torch.from_numpy(st["nodes_i"]), torch.from_numpy(st["nodes_j"])) for st in steps]
    mean_loss = ds.train({"clf_lr": p["clf_lr"]}, loader, StubModel(), clf, opt, scaler, augment=lambda a, b: (a, b))
    final = {n: q.detach().clone() for n, q in clf.named_parameters()}
    return rec, mean_loss, final


def analyse(steps, rec, p):
    """mined indices, masks, scores and losses per step from the recorded hooks; checks the margins (None when one fails)"""
    import torch
    B, k = p["B"], p["k"]
    out = {"hn": [], "keep": [], "scores": [], "losses": []}
    for s, st in enumerate(steps):
        zi, zj = st["z_i"].astype(np.float64), st["z_j"].astype(np.float64)
        sim = zi @ np.concatenate([zi, zj]).T
        srt = -np.sort(-sim, axis=1)[:, :k + 2]
        if np.diff(-srt, axis=1).min() < SIM_GAP:
            return None
        (xi_p, xj_p), (xi_n, xj_n) = rec["clf_in"][2 * s], rec["clf_in"][2 * s + 1]
        x_all = torch.cat([torch.from_numpy(st["nodes_i"]), torch.from_numpy(st["nodes_j"])])
        flat = x_all.reshape(2 * B, -1)
        hn = np.array([int(torch.nonzero((flat == r.reshape(1, -1)).all(1))[0]) for r in xj_n])
        assert torch.equal(xi_p, x_all[:B]) and torch.equal(xj_p, x_all[B:]) and torch.equal(xi_n, x_all[:B].repeat(k, 1, 1))
        hn = hn.reshape(B, k)
        assert (hn == np.argsort(-sim, axis=1, kind="stable")[:, 1:k + 1]).all()
        cand = np.concatenate([np.arange(B) + B, hn.reshape(-1)])
        if np.bincount(cand).max() < 2:
            return None
        pre = torch.cat([rec["fc0_out"][2 * s], rec["fc0_out"][2 * s + 1]])
        if pre.abs().min() < PRE_GAP:
            return None
        fin = torch.cat([rec["fc2_in"][2 * s], rec["fc2_in"][2 * s + 1]])
        fout = torch.cat([rec["fc2_out"][2 * s], rec["fc2_out"][2 * s + 1]])
        keep_bits = np.where(fin.numpy() > 0, fout.numpy() != 0, True)
        sc = torch.cat([rec["scores"][2 * s], rec["scores"][2 * s + 1]])
        crit = torch.nn.BCELoss()
        loss = crit(sc[:B], torch.ones(B, 1)) + crit(sc[B:], torch.zeros(k * B, 1))
        out["hn"].append(hn)
        out["keep"].append(keep_bits)
        out["scores"].append(sc.numpy().reshape(-1))
        out["losses"].append(float(loss))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference-repo", required=True)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    sys.path.insert(0, HERE)
    p = PARAMS
    for seed in range(args.seed, args.seed + 200):
        steps, state = make_case(seed, p), classifier_state(seed, p)
        rec, mean_loss, final = run_reference(args.reference_repo, steps, state, p)
        res = analyse(steps, rec, p)
        if res is not None:
            break
        print(f"seed {seed}: a margin fails, next seed")
    else:
        raise SystemExit("no seed in range meets the margins")
    assert abs(mean_loss - float(np.mean(res["losses"]))) < 1e-6
    z = {"seed": np.array(seed), "params": np.frombuffer(json.dumps(p).encode(), np.uint8), "digest": np.array(digest(steps, state)),
         "hn": np.stack(res["hn"]).astype(np.int64), "keep_bits": np.packbits(np.stack(res["keep"]), axis=-1),
         "scores": np.stack(res["scores"]).astype(np.float32), "losses": np.array(res["losses"]), "mean_loss": np.array(mean_loss)}
    for n in PARAM_NAMES:
        idx = sample_index(seed, tuple(final[n].shape), p)
        z.update(compact("grad0/" + n, rec["grads"][n].numpy(), idx))
        z.update(compact("final/" + n, final[n].numpy(), idx))
    np.savez_compressed(FIXTURE, **z)
    print(f"wrote {FIXTURE} ({os.path.getsize(FIXTURE)} bytes), seed {seed}, losses {res['losses']}")


if __name__ == "__main__":
    main()
