"""Exact filtered search on the flat index (HipFlatIndex.search(x, k, params=SearchParameters(sel=...)),
prag_index_search_filtered) against the definition computed here: a float64 brute force over the stored rows of the
selected subset, row by row in one summation order, ranked by (score, id), faiss padding.  Two float64 summation orders
may disagree in the last bits, so where the returned id differs from the reference's at some rank, both rows must hold
reference scores within 1e-12 (cosine: 1e-7) of each other - a "don't care" near-tie, which must be rare.  D is compared
to float32 of the reference score at rtol 1e-6."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import oracle_np as onp

pytestmark = pytest.mark.gpu

FMAX = np.float32(np.finfo(np.float32).max)


def stored_rows(X, metric, store):
    return onp.store_round(onp.normalize_rows(X) if metric == "cos" else X, store)


def ref_scores(Xs, Q, metric):
    x64 = np.asarray(Xs, np.float64)
    q64 = np.asarray(onp.normalize_rows(Q) if metric == "cos" else Q, np.float64)
    out = np.empty((len(Q), len(Xs)))
    for b in range(len(Q)):
        for c0 in range(0, len(Xs), 1 << 16):
            xs = x64[c0:c0 + (1 << 16)]
            if metric == "l2":
                diff = xs - q64[b]
                out[b, c0:c0 + len(xs)] = np.einsum("nd,nd->n", diff, diff)
            else:
                out[b, c0:c0 + len(xs)] = np.einsum("nd,d->n", xs, q64[b])
    return out


def ref_order(S, member, metric):
    """[B, n_sel] selected row ids of every query in the definition's order."""
    ids = np.nonzero(member)[0]
    out = np.empty((S.shape[0], len(ids)), np.int64)
    for b in range(S.shape[0]):
        s = S[b, ids]
        out[b] = ids[np.lexsort((ids, s if metric == "l2" else -s))]
    return out


def check(D, I, S, order, k, metric, member, id_offset=0):
    """(D, I) of B = len(D) queries against the definition; returns the number of don't-care near-ties."""
    D = D.cpu().numpy() if isinstance(D, torch.Tensor) else np.asarray(D)
    I = I.cpu().numpy() if isinstance(I, torch.Tensor) else np.asarray(I)
    B = D.shape[0]
    assert D.shape == I.shape == (B, k) and D.dtype == np.float32 and I.dtype == np.int64
    n_sel = order.shape[1]
    m = min(k, n_sel)
    tol = 1e-12 if metric != "cos" else 1e-7
    n_dc = 0
    for b in range(B):
        got = I[b, :m] - id_offset
        want = order[b, :m]
        assert np.all(got >= 0) and np.all(got < S.shape[1]), f"query {b}: ids {got[:8]}"
        assert np.all(member[got]), f"query {b}: an unselected row was returned"
        assert len(set(got.tolist())) == m
        diff = np.nonzero(got != want)[0]
        for j in diff:
            s_g, s_w = S[b, got[j]], S[b, want[j]]
            assert abs(s_g - s_w) <= tol * max(1.0, abs(s_w)), \
                f"query {b} rank {j}: got row {got[j]} ({s_g}), want {want[j]} ({s_w})"
        n_dc += len(diff)
        np.testing.assert_allclose(D[b, :m], S[b, got].astype(np.float32), rtol=1e-6, atol=1e-6 if metric == "cos" else 0)
        if m < k:      # faiss padding
            assert np.all(I[b, m:] == -1)
            assert np.all(D[b, m:] == (FMAX if metric == "l2" else -FMAX))
    return n_dc


def selector_cases(N, k_max, rng):
    import probing_rag_amd as pra
    allrows = np.ones(N, bool)
    r50 = rng.random(N) < 0.5
    r01 = rng.random(N) < 0.01
    lo, hi = 37, 37 + max(1, N // 3) + 5          # not aligned to 32 at either end
    rng_m = np.zeros(N, bool)
    rng_m[lo:hi] = True
    one = np.zeros(N, bool)
    one[N // 2] = True
    few_ids = rng.choice(N, min(N, max(1, k_max // 3)), replace=False)
    few = np.zeros(N, bool)
    few[few_ids] = True
    bitmap = np.packbits(r50, bitorder="little")
    return {
        "all": (pra.IDSelectorRange(0, N), allrows),
        "rand50": (pra.IDSelectorBitmap(bitmap), r50),
        "rand1": (pra.IDSelectorBatch(np.nonzero(r01)[0]), r01),
        "range": (pra.IDSelectorRange(lo, hi), rng_m),
        "single": (pra.IDSelectorArray([N // 2]), one),
        "none": (pra.IDSelectorNot(pra.IDSelectorRange(-5, N + 5)), np.zeros(N, bool)),
        "fewer_than_k": (pra.IDSelectorBatch(few_ids), few),
    }


PARITY = [(m, s, d) for m in ("l2", "ip", "cos") for s in ("f32", "f16") for d in (64, 768, 1024)]


@pytest.mark.parametrize("metric,store,d", PARITY)
def test_filter_parity(metric, store, d, monkeypatch):
    import probing_rag_amd as pra
    N = 3001
    X = onp.synth_rows(11 + d, 0, N, d)
    Q = onp.synth_rows(5 + d, 0, 300, d)
    ix = pra.HipFlatIndex(d, metric, store)
    ix.add(X)
    S = ref_scores(stored_rows(X, metric, store), Q, metric)
    rng = np.random.default_rng(d)
    n_dc = 0
    for name, (sel, member) in selector_cases(N, 100, rng).items():
        order = ref_order(S, member, metric)
        p = pra.SearchParameters(sel=sel)
        for B in (1, 5, 64, 300):
            for k in (1, 10, 100):
                if name in ("range", "rand1") and B == 300 and k == 100 and d == 1024:
                    continue    # (time: the same shapes run at the other dimensions)
                results = []
                for path in ("1", "2"):
                    if path == "1" and k > 26:
                        continue            # the masked scan has no deep lists: k > 26 always gathers
                    monkeypatch.setenv("PRAG_FILTER_PATH", path)
                    D, I = ix.search(Q[:B], k, params=p)
                    info = ix.last_filter()
                    assert info["n_selected"] == int(member.sum())
                    assert info["path"] == int(path)
                    n_dc += check(D, I, S[:B], order[:B], k, metric, member)
                    results.append((D, I))
                if len(results) == 2:       # both paths: the same (D, I)
                    assert np.array_equal(results[0][0], results[1][0]) and np.array_equal(results[0][1], results[1][1])
    assert n_dc <= 4, f"{n_dc} don't-care near-ties"


def test_filter_identities(monkeypatch):
    import probing_rag_amd as pra
    d, N, B, k = 768, 20011, 16, 10
    X = onp.synth_rows(3, 0, N, d)
    Q = torch.from_numpy(onp.synth_rows(4, 0, B, d)).cuda()
    ix = pra.HipFlatIndex(d, "l2", "f16")
    ix.add(X)
    D0, I0 = ix.search(Q, k)
    assert ix.last_exact_fallbacks() == 0
    for path in ("", "1", "2"):
        monkeypatch.setenv("PRAG_FILTER_PATH", path)
        D, I = ix.search(Q, k, params=pra.SearchParameters(sel=pra.IDSelectorRange(0, N)))
        info = ix.last_filter()
        assert info["n_flagged"] == 0 and info["n_selected"] == N and info["n_tiles"] == (N + 31) // 32
        assert torch.equal(D, D0) and torch.equal(I, I0), path
    monkeypatch.delenv("PRAG_FILTER_PATH")
    # a subset gives what search gives on a fresh index of those rows, ids mapped back
    rng = np.random.default_rng(8)
    for frac in (0.03, 0.6):
        sub = np.sort(rng.choice(N, int(frac * N), replace=False))
        D, I = ix.search(Q, k, params=pra.SearchParameters(sel=pra.IDSelectorBatch(sub)))
        fresh = pra.HipFlatIndex(d, "l2", "f16")
        fresh.add(X[sub])
        Ds, Is = fresh.search(Q, k)
        assert torch.equal(D, Ds)
        assert torch.equal(I, torch.from_numpy(sub).cuda()[Is])


def test_filter_paths_and_auto_rule_multistep(monkeypatch):
    """300 017 rows x 128 fp16: every workgroup of the masked scan walks several tiles.  Contiguous and random
    selectors against the definition on both paths; the auto rule gathers a 0.1 % selection and scans a 50 % one."""
    import probing_rag_amd as pra
    d, N, B, k = 128, 300017, 64, 10
    X = onp.synth_rows(21, 0, N, d)
    Q = onp.synth_rows(22, 0, B, d)
    ix = pra.HipFlatIndex(d, "l2", "f16")
    ix.add(X)
    rng = np.random.default_rng(1)
    S = ref_scores(stored_rows(X, "l2", "f16"), Q[:8], "l2")
    contiguous = np.zeros(N, bool)
    contiguous[1000:1000 + N // 8] = True
    rand = rng.random(N) < 0.5
    for member in (contiguous, rand):
        sel = pra.IDSelectorBitmap(np.packbits(member, bitorder="little"))
        order = ref_order(S, member, "l2")
        out = []
        for path in ("1", "2"):
            monkeypatch.setenv("PRAG_FILTER_PATH", path)
            D, I = ix.search(Q[:8], k, params=pra.SearchParameters(sel=sel))
            assert ix.last_filter()["path"] == int(path)
            assert check(D, I, S, order, k, "l2", member) <= 1
            out.append((D, I))
        assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])
    monkeypatch.delenv("PRAG_FILTER_PATH")
    tiny = rng.choice(N, N // 1000, replace=False)
    ix.search(Q, k, params=pra.SearchParameters(sel=pra.IDSelectorBatch(tiny)))
    assert ix.last_filter()["path"] == 2
    half = pra.IDSelectorBitmap(np.packbits(rand, bitorder="little"))
    ix.search(Q, k, params=pra.SearchParameters(sel=half))
    info = ix.last_filter()
    assert info["path"] == 1 and info["n_tiles"] == (N + 31) // 32


def test_filter_certificate_fallback(monkeypatch):
    """Clustered near-duplicate rows: the masked scan cannot certify the queries, the gathered float64 path
    recomputes them, and the result is exact."""
    import probing_rag_amd as pra
    d, N, C = 768, 60000, 24
    rng = np.random.default_rng(5)
    centres = rng.standard_normal((C, d)).astype(np.float32)
    X = (centres[rng.integers(0, C, N)] + 2e-3 * rng.standard_normal((N, d))).astype(np.float32)
    Q = (centres[:6] + 1e-3 * rng.standard_normal((6, d))).astype(np.float32)
    member = rng.random(N) < 0.4
    monkeypatch.setenv("PRAG_FILTER_PATH", "1")
    for metric, store in (("l2", "f16"), ("ip", "f32")):
        ix = pra.HipFlatIndex(d, metric, store)
        ix.add(X)
        S = ref_scores(stored_rows(X, metric, store), Q, metric)
        D, I = ix.search(Q, 10, params=pra.SearchParameters(sel=pra.IDSelectorBitmap(np.packbits(member, bitorder="little"))))
        info = ix.last_filter()
        assert info["path"] == 1 and info["n_flagged"] > 0, info
        check(D, I, S, ref_order(S, member, metric), 10, metric, member)


def test_filter_io_forms_and_shards():
    import probing_rag_amd as pra
    d, N, B, k = 256, 9001, 12, 10
    X = onp.synth_rows(41, 0, N, d)
    Q = onp.synth_rows(42, 0, B, d)
    rng = np.random.default_rng(4)
    member = rng.random(N) < 0.3
    ix = pra.HipFlatIndex(d, "ip", "f16")
    ix.add(X)
    S = ref_scores(stored_rows(X, "ip", "f16"), Q, "ip")
    order = ref_order(S, member, "ip")
    off = 1000
    # selector ids are search's ids (row + id_offset): shift the membership by the offset
    bm_host = np.packbits(np.concatenate([np.zeros(off, bool), member]), bitorder="little")
    sel_h = pra.IDSelectorBitmap(bm_host)
    sel_d = pra.IDSelectorBitmap(torch.from_numpy(bm_host).cuda())
    Dh, Ih = ix.search(Q, k, id_offset=off, params=pra.SearchParameters(sel=sel_h))
    assert isinstance(Dh, np.ndarray)
    check(Dh, Ih, S, order, k, "ip", member, id_offset=off)
    Qd = torch.from_numpy(Q).cuda()
    for sel in (sel_h, sel_d):
        Dd, Id = ix.search(Qd, k, id_offset=off, params=pra.SearchParameters(sel=sel))
        assert Dd.is_cuda and Id.is_cuda
        assert np.array_equal(Dd.cpu().numpy(), Dh) and np.array_equal(Id.cpu().numpy(), Ih)
    # two row shards on one GPU: each searches its window of the global selector with its offset; merge_topk
    cut = 4321                                    # (not a multiple of 8 or 32: the CUDA bitmap window is shifted)
    sel_g = pra.IDSelectorBitmap(torch.from_numpy(np.packbits(member, bitorder="little")).cuda())
    parts = []
    for lo, hi in ((0, cut), (cut, N)):
        sh = pra.HipFlatIndex(d, "ip", "f16")
        sh.add(X[lo:hi])
        parts.append(sh.search(Qd, k, id_offset=lo, params=pra.SearchParameters(sel=sel_g)))
    Dm, Im = pra.merge_topk(torch.stack([p[0] for p in parts]), torch.stack([p[1] for p in parts]), k, "ip")
    D1, I1 = ix.search(Qd, k, params=pra.SearchParameters(sel=sel_g))
    assert torch.equal(Dm, D1) and torch.equal(Im, I1)


def test_filter_leaves_search_state():
    import probing_rag_amd as pra
    d, N, B, k = 768, 12007, 8, 5
    X = onp.synth_rows(51, 0, N, d)
    Q = torch.from_numpy(onp.synth_rows(52, 0, B, d)).cuda()
    ix = pra.HipFlatIndex(d, "l2", "f16")
    ix.add(X)
    D0, I0 = ix.search(Q, k)
    plan0 = ix.last_plan()
    for kk in (5, 40):
        ix.search(Q, kk, params=pra.SearchParameters(sel=pra.IDSelectorRange(100, 9000)))
    D1, I1 = ix.search(Q, k)
    assert torch.equal(D0, D1) and torch.equal(I0, I1)
    assert ix.last_plan() == plan0


def test_filter_errors_and_empty_index():
    import probing_rag_amd as pra
    from probing_rag_amd import _lib
    d = 64
    ix = pra.HipFlatIndex(d, "l2", "f16")
    Q = onp.synth_rows(1, 0, 3, d)
    # ntotal == 0: all padding
    D, I = ix.search(Q, 4, params=pra.SearchParameters(sel=pra.IDSelectorRange(0, 10)))
    assert np.all(I == -1) and np.all(D == FMAX)
    ix.add(onp.synth_rows(2, 0, 100, d))
    p = pra.SearchParameters(sel=pra.IDSelectorRange(0, 50))
    with pytest.raises(ValueError):
        ix.search(Q, 4, tagged=True, params=p)
    for k in (0, 912):
        with pytest.raises(_lib.PragError):
            ix.search(Q, k, params=p)
    # too few bitmap words: 100 rows need 4
    words = np.zeros(3, np.uint32)
    D = np.empty((3, 4), np.float32)
    I = np.empty((3, 4), np.int64)
    q = np.ascontiguousarray(Q, np.float32)
    rc = _lib.lib().prag_index_search_filtered(ix._h, ctypes.c_void_p(q.ctypes.data), 3, 4, 0,
                                               ctypes.c_void_p(words.ctypes.data), 3, 0, ctypes.c_void_p(D.ctypes.data),
                                               ctypes.c_void_p(I.ctypes.data), 0, None)
    assert rc == -1 and b"n_words" in _lib.lib().prag_last_error()
    # B = 0 writes nothing
    D, I = ix.search(np.zeros((0, d), np.float32), 4, params=p)
    assert D.shape == (0, 4)
