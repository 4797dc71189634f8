"""Shared inputs, the fp64 oracle and the bounds of the LDA held-out fold-in
tests (test_lda_foldin_cpu.py, test_lda_foldin_gpu.py).

The oracle is a per-document float64 loop over the definition, written
without ops or mlapps.heldout:

  phi[w,k] = (n_wk + beta) / (n_k + V beta)
  step:   m_k = sum_obs c theta_k phi[w,k] / sum_j theta_j phi[w,j]
          theta_k = (m_k + alpha) / (N_obs + K alpha)
  score:  ll = sum_scored c log sum_k theta_k phi[w,k]

Bounds, u = 2^-24 (the float32 unit roundoff). Every term is positive, so
every bound is relative and a float32 sum of k terms in ANY order is within
(k - 1) u of the exact sum of its (already rounded) terms. To first order:

* A term theta_k phi[w,k], evaluated from float32 theta: beta rounded to
  float32 moves n + beta by at most u, the addition rounds (u); the
  denominator n_k + V beta has the rounding of V beta, of the addition and of
  the reciprocal (3 u); two multiplications put the three factors together
  (2 u): 7 u. The K-term sum adds (K - 1) u:
      total = sum_k theta_k phi[w,k]   within (K + 6) u.
* One fold-in step from a given float32 theta: r_k = c * term / total has the
  term's 7 u, the total's (K + 6) u and two more roundings, (K + 15) u; m_k
  sums P such values, (P - 1) u; m_k + alpha has alpha's rounding and the
  addition's (2 u); the denominator N_obs + K alpha a product and a sum, and
  then the division (3 u): (K + P + 19) u. The bound used is the roomier
      (2 K + P + 20) u   per theta entry, P the observed pair count.
* ll: each scored pair contributes c log(total). The total's error moves the
  logarithm by (K + 6) u ABSOLUTE; logf is good to 2 ulp = 4 u |log total|
  and the product with c rounds once more (inside the 4 u); the S-term sum in
  float32 adds at most S u sum|terms|:
      sum_pairs c ((K + 6) u + 4 u |log total|) + S u sum|terms|.
* theta sums to one: sum_k m_k = N_obs up to the totals' rounding, so
      |sum_k theta_k - 1| <= 2 (K + 4) u
  as the specification of the kernel states it.

Each bound is applied with a factor 2 for the second-order terms (SAFETY).
None of this is tuned to an implementation.
"""

import math
from collections import Counter
from pathlib import Path

import numpy as np
import torch

from harmony_amd.config import JobConfig

U = 2.0 ** -24
SAFETY = 2.0
V = 128
ALPHA, BETA = 0.1, 0.01
SHAPE_KS = (8, 64, 96, 320, 576, 1024)
ZERO_ROW = 5                      # the word whose row is all zero


# ----------------------------------------------------------------- inputs

def split_pairs(docs, device="cpu"):
    """Document completion by hand: tokens at even positions observed, at
    odd positions scored, each half as (word, count) sorted by word.
    -> (obs_ptr, obs_word, obs_cnt, sc_ptr, sc_word, sc_cnt)."""
    out = []
    for first in (0, 1):
        ptr, word, cnt = [0], [], []
        for doc in docs:
            c = Counter(doc[first::2])
            for w in sorted(c):
                word.append(w)
                cnt.append(c[w])
            ptr.append(len(word))
        out += [torch.tensor(ptr, dtype=torch.int64, device=device),
                torch.tensor(word, dtype=torch.int64, device=device),
                torch.tensor(cnt, dtype=torch.int32, device=device)]
    return tuple(out)


def shape_docs():
    """13 documents over V = 128 (not a multiple of 8 or 4 per workgroup):
    one of 2 tokens, one of 200 tokens of a single word (one pair of count
    100 per half), mixed lengths 3..64, word V - 1 and the all-zero row."""
    g = torch.Generator().manual_seed(1357)
    docs = [[7, 9], [33] * 200]
    for n in (3, 4, 5, 17, 31, 32, 33, 47, 63, 64):
        docs.append(torch.randint(0, V, (n,), generator=g).tolist())
    docs.append([V - 1, ZERO_ROW, V - 1, ZERO_ROW, 0, V - 1, ZERO_ROW])
    assert len(docs) == 13
    return docs


def random_table(K, seed=11):
    """int32 [V + 1, K]: skewed counts, row ZERO_ROW all zero, the summary
    row the column sums."""
    g = torch.Generator().manual_seed(seed + K)
    t = torch.randint(0, 50, (V + 1, K), generator=g, dtype=torch.int32)
    t = t * (torch.rand(V + 1, K, generator=g) < 0.3).to(torch.int32)
    t[ZERO_ROW] = 0
    t[V] = t[:V].sum(dim=0)
    return t


def planted_table():
    """8 topics x 16 private words, counts 1000."""
    t = torch.zeros(V + 1, 8, dtype=torch.int32)
    for k in range(8):
        t[16 * k:16 * (k + 1), k] = 1000
    t[V] = t[:V].sum(dim=0)
    return t


def planted_docs(n_docs, n_tokens, seed):
    """Document i draws n_tokens from the 16 words of topic i % 8."""
    g = torch.Generator().manual_seed(seed)
    return [(16 * (i % 8)
             + torch.randint(0, 16, (n_tokens,), generator=g)).tolist()
            for i in range(n_docs)]


def write_docs(path, docs, scheme=""):
    Path(path).write_text(
        "\n".join(" ".join(str(w) for w in d) for d in docs) + "\n")
    return scheme + str(path)


def planted_files(tmp_path):
    """(training file of 64 documents x 32 tokens, held-out file of 13
    documents x 24 tokens, the held-out documents)."""
    held = planted_docs(13, 24, seed=99)
    return (write_docs(tmp_path / "train", planted_docs(64, 32, seed=98)),
            write_docs(tmp_path / "held_out", held), held)


def lda_job(job_id, train, test, epochs=8, **kw):
    args = {"input": str(train), "num_topics": 8, "num_vocabs": V,
            "sampler": "exact", "alpha": ALPHA, "beta": BETA}
    if test is not None:
        args["test_data_path"] = str(test)
    job_kw = {k: kw.pop(k) for k in list(kw)
              if k in ("model_chkp_per_epoch", "offline_model_eval",
                       "chkp_path")}
    args.update(kw)
    return JobConfig(job_id=job_id, app="lda", max_num_epochs=epochs,
                     num_mini_batches=2, app_args=args, **job_kw)


def recomputed(trainer, held, iters=20):
    """(perplexity, log-likelihood) from ops.lda_foldin on the trainer's
    pulled table and the by-hand split of the held-out documents, reduced
    as evaluate_test is specified to: fp64 sum of the fp32 ll, one divide."""
    from harmony_amd import ops

    a = trainer.a
    nv = a["num_vocabs"]
    full = trainer.accessor.table.pull_all()[:nv + 1]
    pairs = split_pairs(held, device=full.device)
    _theta, ll = ops.lda_foldin(full[:nv], full[nv], *pairs, a["alpha"],
                                a["beta"], nv, iters)
    total = float(ll.double().sum())
    tokens = sum(len(d) // 2 for d in held)
    return math.exp(-total / tokens), total


# ----------------------------------------------------------------- oracle

def phi64(table, num_vocabs=V, beta=BETA):
    t = table.cpu().numpy().astype(np.float64)
    return (t[:num_vocabs] + beta) / (t[num_vocabs] + num_vocabs * beta)


def doc_pairs(ptr, word, cnt, d):
    lo, hi = int(ptr[d]), int(ptr[d + 1])
    return (word[lo:hi].cpu().numpy(),
            cnt[lo:hi].cpu().numpy().astype(np.float64))


def step64(theta, words, counts, phi, alpha=ALPHA):
    """One fold-in step of one document from theta (float64 [K])."""
    K = theta.shape[0]
    m = np.zeros(K)
    for w, c in zip(words, counts):
        val = theta * phi[w]
        m += c * val / val.sum()
    return (m + alpha) / (counts.sum() + K * alpha)


def score64(theta, words, counts, phi):
    """(ll, its bound for a float32 evaluation from this theta)."""
    K = theta.shape[0]
    ll = bound = mag = 0.0
    for w, c in zip(words, counts):
        lt = math.log(float((theta * phi[w]).sum()))
        ll += c * lt
        mag += abs(c * lt)
        bound += c * ((K + 6) * U + 4 * U * abs(lt))
    return ll, SAFETY * (bound + len(words) * U * mag)


def step_bound(K, P):
    return SAFETY * (2 * K + P + 20) * U


def foldin64(table, pairs, iters, num_vocabs=V, alpha=ALPHA, beta=BETA):
    """From scratch in float64: (theta [D, K], ll [D])."""
    phi = phi64(table, num_vocabs, beta)
    K = phi.shape[1]
    D = pairs[0].shape[0] - 1
    thetas, lls = np.zeros((D, K)), np.zeros(D)
    for d in range(D):
        ow, oc = doc_pairs(*pairs[:3], d)
        theta = np.full(K, 1.0 / K)
        for _ in range(iters):
            theta = step64(theta, ow, oc, phi, alpha)
        thetas[d] = theta
        lls[d] = score64(theta, *doc_pairs(*pairs[3:], d), phi)[0]
    return thetas, lls


# ----------------------------------------------------------------- checks

def run_op(table, pairs, iters, device, num_vocabs=V, alpha=ALPHA,
           beta=BETA):
    from harmony_amd import ops

    t = table.to(device)
    theta, ll = ops.lda_foldin(t[:num_vocabs], t[num_vocabs],
                               *[p.to(device) for p in pairs], alpha, beta,
                               num_vocabs, iters)
    assert theta.dtype == torch.float32 and ll.dtype == torch.float32
    assert theta.device.type == ll.device.type == torch.device(device).type
    return theta.cpu(), ll.cpu()


def check_rows_sum_to_one(theta):
    K = theta.shape[1]
    err = float((theta.double().sum(dim=1) - 1).abs().max())
    print(f"  K={K}: |sum theta - 1| max {err:.3e}, "
          f"bound {2 * (K + 4) * U:.3e}")
    assert err <= 2 * (K + 4) * U


def check_chain(table, pairs, device, label=""):
    """Checks 1 and 2: iters = 0..5 of the op; theta_0 exactly 1/K, every
    theta_{I+1} within one step's bound of the fp64 step from the op's own
    theta_I, every ll within its bound of the fp64 score of the op's own
    theta_I, every theta row summing to one."""
    phi = phi64(table)
    K = phi.shape[1]
    D = pairs[0].shape[0] - 1
    runs = [run_op(table, pairs, i, device) for i in range(6)]
    theta0 = runs[0][0]
    assert theta0.shape == (D, K) and runs[0][1].shape == (D,)
    assert bool((theta0 == float(np.float32(1) / np.float32(K))).all())
    worst_t = worst_l = 0.0
    for i in range(5):
        theta_i, ll_i = runs[i]
        theta_n = runs[i + 1][0].double().numpy()
        check_rows_sum_to_one(runs[i + 1][0])
        for d in range(D):
            ow, oc = doc_pairs(*pairs[:3], d)
            th = theta_i[d].double().numpy()
            want = step64(th, ow, oc, phi)
            rel = float(np.abs(theta_n[d] / want - 1).max())
            tb = step_bound(K, len(ow))
            worst_t = max(worst_t, rel / tb)
            assert rel <= tb, (label, "theta", i, d, rel, tb)
            ll64, lb = score64(th, *doc_pairs(*pairs[3:], d), phi)
            err = abs(float(ll_i[d]) - ll64)
            worst_l = max(worst_l, err / lb)
            assert err <= lb, (label, "ll", i, d, err, lb)
    print(f"{label} K={K} D={D} on {device}: worst theta error "
          f"{worst_t:.3f} of its bound, worst ll error {worst_l:.3f} of its")


def end_to_end_error(table, pairs, device, label=""):
    """Printed, not asserted: iters = 20 against float64 from scratch."""
    theta, ll = run_op(table, pairs, 20, device)
    t64, l64 = foldin64(table, pairs, 20)
    te = float(np.abs(theta.double().numpy() / t64 - 1).max())
    le = float(np.abs(ll.double().numpy() - l64).max())
    lr = float(np.abs(ll.double().numpy() / np.where(l64 == 0, 1, l64)
                      - 1).max())
    print(f"{label} K={theta.shape[1]} on {device}, iters 20, fp32 against "
          f"fp64 from scratch: theta max rel {te:.3e}, ll max abs {le:.3e} "
          f"(rel {lr:.3e})")
    return te, le


def equal_rows_tables(K=8):
    """Every word row 3 with the summary row 3 V, and the all-zero table:
    phi = 1/V in both, whatever theta is."""
    a = torch.full((V + 1, K), 3, dtype=torch.int32)
    a[V] = 3 * V
    return {"threes": a, "zeros": torch.zeros(V + 1, K, dtype=torch.int32)}


def check_perplexity_is_v(table, pairs, device, num_vocabs=V, iters=(0, 20)):
    """Check 3: exp(-sum ll / tokens) = V within the ll bound."""
    tokens = int(pairs[5].sum())
    K = table.shape[1]
    D = pairs[0].shape[0] - 1
    lv = math.log(num_vocabs)
    # every total is 1/V: the ll bound in closed form
    bound = 0.0
    for d in range(D):
        _w, c = doc_pairs(*pairs[3:], d)
        bound += SAFETY * (float(c.sum()) * ((K + 6) * U + 4 * U * lv)
                           + len(c) * U * float(c.sum()) * lv)
    for it in iters:
        _theta, ll = run_op(table, pairs, it, device, num_vocabs=num_vocabs)
        total = float(ll.double().sum())
        ppl = math.exp(-total / tokens)
        print(f"  iters {it}: perplexity {ppl!r}, V {num_vocabs}, ll error "
              f"{abs(total + tokens * lv):.3e}, bound {bound:.3e}")
        assert abs(total + tokens * lv) <= bound
