"""Exact range search on the flat index (HipFlatIndex.range_search, prag_index_range_search) against a float64
brute force defined here: row by row, one summation order, over the rows the index stores.  Rows whose reference
score lies within 1e-12 * max(1, |radius|) of the radius are "don't care" for membership (two float64 summation
orders may disagree there); they must be rare (at most 2 per case), everything else is compared exactly.  Cosine
queries are normalised by the index and by the reference in different summation orders, so a query component may
differ in its last bit: there the band is 1e-7 and D is compared to 1e-6 (the boundary test compares cosine D with
search's bit for bit)."""
import numpy as np
import pytest
import torch

from oracle import oracle_np as onp

pytestmark = pytest.mark.gpu

METRICS = {"l2": onp.METRIC_L2, "ip": onp.METRIC_IP, "cos": onp.METRIC_COS}


def stored_rows(X, metric, store):
    return onp.store_round(onp.normalize_rows(X) if metric == "cos" else X, store)


def ref_scores(Xs, Q, metric):
    """float64 [B, N] over the stored rows Xs: sum of (q - x)^2 (L2) or q . x (IP / COS, query normalised)."""
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


def pick_radius(S, metric, per_query):
    """float32 radius with about `per_query` rows in range per query (0: none at all)."""
    if per_query == 0 or S.shape[1] == 0:
        return -1.0 if metric == "l2" else 1e30
    k = min(per_query, S.shape[1])
    kth = np.sort(S, axis=1)[:, k - 1] if metric == "l2" else -np.sort(-S, axis=1)[:, k - 1]
    return float(np.float32(np.median(kth)))


def check_range(lims, D, I, S, radius, metric, id_offset=0, d_exact=True):
    """Exact comparison with the definition outside the don't-care band; returns the number of results."""
    B, N = S.shape
    r = float(np.float32(radius))
    lims, D, I = (t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t) for t in (lims, D, I))
    assert lims.dtype == np.int64 and lims.shape == (B + 1,) and lims[0] == 0
    assert np.all(np.diff(lims) >= 0) and len(D) == len(I) == lims[B]
    assert D.dtype == np.float32 and I.dtype == np.int64
    tol = (1e-12 if metric != "cos" else 1e-7) * max(1.0, abs(r))
    n_dc = 0
    for b in range(B):
        ids = I[lims[b]:lims[b + 1]] - id_offset
        assert np.all(np.diff(ids) > 0), f"query {b}: ids not strictly ascending"
        assert len(ids) == 0 or (ids[0] >= 0 and ids[-1] < N)
        s = S[b]
        dc = np.abs(s - r) <= tol
        n_dc += int(dc.sum())
        want = (s < r) if metric == "l2" else (s > r)
        got = np.zeros(N, bool)
        got[ids] = True
        bad = np.nonzero((got != want) & ~dc)[0]
        assert len(bad) == 0, f"query {b}: membership differs at rows {bad[:8]} (scores {s[bad[:8]]}, radius {r})"
        Dw = s[ids].astype(np.float32)
        Dg = D[lims[b]:lims[b + 1]]
        if d_exact:
            assert np.array_equal(Dg, Dw), f"query {b}: D differs"
        else:   # cosine: the reference normalises the query in its own summation order
            np.testing.assert_allclose(Dg, Dw, rtol=1e-6, atol=1e-6)
    # (cosine: the band also absorbs the last-bit differences of the two query normalisations, and so holds more rows
    #  when there are many results)
    assert n_dc <= (2 if metric != "cos" else 2 + int(lims[B]) // 10000), f"{n_dc} rows in the don't-care band"
    return int(lims[B])


# (metric, store, d, N, B, rows): every metric and store, d in {64, 768, 1536}, N in {0, 1, 31, 33, 10 007, 300 017},
# B in {1, 5, 64, 200}
PARITY = [
    ("l2", "f32", 768, 10007, 5, "synth"),
    ("l2", "f16", 768, 10007, 5, "embed"),
    ("ip", "f32", 768, 10007, 5, "synth"),
    ("ip", "f16", 768, 10007, 64, "synth"),
    ("cos", "f32", 768, 10007, 5, "embed"),
    ("cos", "f16", 768, 10007, 5, "synth"),
    ("l2", "f16", 64, 0, 5, "synth"),
    ("ip", "f32", 64, 1, 1, "synth"),
    ("l2", "f16", 64, 31, 64, "synth"),
    ("ip", "f16", 1536, 33, 5, "synth"),
    ("l2", "f32", 1536, 10007, 64, "embed"),
    ("cos", "f16", 1536, 10007, 200, "synth"),
    ("l2", "f16", 64, 10007, 200, "synth"),
    ("l2", "f16", 64, 300017, 64, "synth"),
    ("ip", "f32", 64, 300017, 5, "synth"),
    ("l2", "f16", 768, 300017, 1, "embed"),
]


def make_rows(kind, seed, N, d):
    if N == 0:
        return np.zeros((0, d), np.float32)
    return onp.synth_rows(seed, 0, N, d) if kind == "synth" else onp.embedding_like_rows(seed, 0, N, d)


def make_queries(kind, seed, B, d, X):
    if kind == "embed" and len(X):    # queries shaped like the rows (near the corpus)
        return onp.embedding_like_rows(seed + 1000, 0, B, d)
    return onp.synth_rows(seed, 0, B, d)


@pytest.mark.parametrize("metric,store,d,N,B,kind", PARITY)
def test_range_parity(metric, store, d, N, B, kind):
    import probing_rag_amd as pra
    X = make_rows(kind, 11 + d, N, d)
    Q = make_queries(kind, 5, B, d, X)
    ix = pra.HipFlatIndex(d, metric, store)
    if N:
        ix.add(X)
    S = ref_scores(stored_rows(X, metric, store), Q, metric)
    for per_query in (0, 10, 2000):
        r = pick_radius(S, metric, per_query)
        lims, D, I = ix.range_search(Q, r)
        assert isinstance(lims, np.ndarray) and isinstance(D, np.ndarray) and isinstance(I, np.ndarray)
        n = check_range(lims, D, I, S, r, metric, d_exact=metric != "cos")
        if per_query == 0 or N == 0:
            assert n == 0
        elif N >= 10:
            assert n >= B   # the radius is the median of the per-query depth: something to compare


@pytest.mark.parametrize("metric,store", [("l2", "f16"), ("l2", "f32"), ("ip", "f16"), ("cos", "f32")])
def test_range_boundary_radius_matches_search(metric, store):
    """radius = nextafter(D[:, k-1]) of search(q, k): every id search returned is in range with a bit-identical D;
    every extra row ties with the k-th result."""
    import probing_rag_amd as pra
    d, N, k = 768, 20011, 10
    X = onp.embedding_like_rows(3, 0, N, d)
    Q = onp.embedding_like_rows(1003, 0, 8, d)
    ix = pra.HipFlatIndex(d, metric, store)
    ix.add(X)
    Ds, Is = ix.search(Q, k)
    for b in range(len(Q)):
        kth = Ds[b, k - 1]
        r = np.nextafter(kth, np.float32(np.inf) if metric == "l2" else np.float32(-np.inf))
        lims, D, I = ix.range_search(Q[b:b + 1], float(r))
        pos = {int(i): j for j, i in enumerate(I)}
        for j in range(k):
            assert int(Is[b, j]) in pos, (b, j)
            assert D[pos[int(Is[b, j])]].tobytes() == Ds[b, j].tobytes(), (b, j)
        extra = np.setdiff1d(I, Is[b])
        for i in extra:
            assert D[pos[int(i)]] in (kth, np.float32(r)), (b, int(i), D[pos[int(i)]], kth)


def test_range_growth_path():
    """1.6 M results (more than the 2^20 candidates a handle starts with): the store grows and the result is complete
    and exact; a small range search on the same handle afterwards is still exact."""
    import probing_rag_amd as pra
    d, N, B = 64, 200003, 8
    X = onp.synth_rows(21, 0, N, d)
    Q = onp.synth_rows(22, 0, B, d)
    ix = pra.HipFlatIndex(d, "l2", "f16")
    ix.add(X)
    S = ref_scores(stored_rows(X, "l2", "f16"), Q, "l2")
    r = float(np.finfo(np.float32).max)
    lims, D, I = ix.range_search(Q, r)
    assert np.array_equal(lims, np.arange(B + 1, dtype=np.int64) * N)
    assert np.array_equal(I, np.tile(np.arange(N, dtype=np.int64), B))
    check_range(lims, D, I, S, r, "l2")
    r2 = pick_radius(S, "l2", 10)
    lims, D, I = ix.range_search(Q, r2)
    check_range(lims, D, I, S, r2, "l2")


def test_range_dense_near_duplicates():
    """Clustered rows: thousands of rows share a centre, many of them inside the selection's error band around the
    radius - the float64 rerank decides them; the result is exact."""
    import probing_rag_amd as pra
    d, N, C = 768, 60000, 24
    rng = np.random.default_rng(5)
    centres = rng.standard_normal((C, d)).astype(np.float32)
    X = (centres[rng.integers(0, C, N)] + 2e-3 * rng.standard_normal((N, d))).astype(np.float32)
    Q = (centres[:6] + 1e-3 * rng.standard_normal((6, d))).astype(np.float32)
    for metric, store in (("l2", "f16"), ("ip", "f32")):
        ix = pra.HipFlatIndex(d, metric, store)
        ix.add(X)
        S = ref_scores(stored_rows(X, metric, store), Q, metric)
        for per_query in (10, 2000):
            r = pick_radius(S, metric, per_query)
            lims, D, I = ix.range_search(Q, r)
            check_range(lims, D, I, S, r, metric)


def test_range_host_device_io_and_shards():
    import probing_rag_amd as pra
    d, N, B = 768, 30011, 16
    X = onp.synth_rows(31, 0, N, d)
    Q = onp.synth_rows(32, 0, B, d)
    ix = pra.HipFlatIndex(d, "l2", "f16")
    ix.add(X)
    S = ref_scores(stored_rows(X, "l2", "f16"), Q, "l2")
    r = pick_radius(S, "l2", 300)
    lims_h, D_h, I_h = ix.range_search(Q, r, id_offset=7)
    lims_d, D_d, I_d = ix.range_search(torch.from_numpy(Q).cuda(), r, id_offset=7)
    assert isinstance(lims_d, np.ndarray) and D_d.is_cuda and I_d.is_cuda and D_d.device == ix.device
    assert np.array_equal(lims_h, lims_d)
    assert np.array_equal(D_h, D_d.cpu().numpy()) and np.array_equal(I_h, I_d.cpu().numpy())
    check_range(lims_h, D_h, I_h, S, r, "l2", id_offset=7)
    # two row shards on one GPU with their id offsets, concatenated per query == the unsharded result
    cut = 12345
    parts = []
    for lo, hi in ((0, cut), (cut, N)):
        sh = pra.HipFlatIndex(d, "l2", "f16")
        sh.add(X[lo:hi])
        parts.append(sh.range_search(Q, r, id_offset=lo))
    lims, D, I = [0], [], []
    for b in range(B):
        for pl, pD, pI in parts:
            D.append(pD[pl[b]:pl[b + 1]])
            I.append(pI[pl[b]:pl[b + 1]])
        lims.append(lims[-1] + sum(pl[b + 1] - pl[b] for pl, _, _ in parts))
    ix0 = pra.HipFlatIndex(d, "l2", "f16")
    ix0.add(X)
    l0, D0, I0 = ix0.range_search(Q, r)
    assert np.array_equal(np.array(lims), l0)
    assert np.array_equal(np.concatenate(D), D0) and np.array_equal(np.concatenate(I), I0)


def test_range_search_leaves_search_untouched():
    import probing_rag_amd as pra
    from probing_rag_amd import _lib
    d, N = 768, 50000
    X = onp.synth_rows(41, 0, N, d)
    Q = onp.synth_rows(42, 0, 32, d)
    ix = pra.HipFlatIndex(d, "l2", "f16")
    ix.add(X)
    D1, I1 = ix.search(Q, 10)
    lims, _, _ = ix.range_search(Q, float(np.median(D1[:, 9])))
    assert lims[-1] > 0
    D2, I2 = ix.search(Q, 10)
    assert np.array_equal(I1, I2) and D1.tobytes() == D2.tobytes()
    # the two-call shape: a count that does not match the last range search is refused
    import ctypes
    n = int(lims[-1])
    Dh, Ih = np.empty(n + 1, np.float32), np.empty(n + 1, np.int64)
    rc = _lib.lib().prag_index_range_result(ix._h, ctypes.c_void_p(Dh.ctypes.data), ctypes.c_void_p(Ih.ctypes.data),
                                            n + 1, 0, None)
    assert rc == -1
    assert _lib.lib().prag_index_range_result(ix._h, ctypes.c_void_p(Dh.ctypes.data), ctypes.c_void_p(Ih.ctypes.data),
                                              n, 0, None) == 0
