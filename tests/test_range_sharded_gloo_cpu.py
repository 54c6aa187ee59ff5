"""CPU, world_size 2, gloo: ShardedFlatIndex.range_search - per-rank range search of a contiguous shard with its
global id offset, all-gather of the per-query counts and of the padded results, concatenation in rank order - driven
with a NumPy engine standing in for the local shard (the product's only engine is HIP)."""
import os
import socket

import numpy as np
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from oracle import oracle_np as onp


def ref_scores(X, Q, metric):
    """float64 [B, N], row by row in one summation order (what the index ranks by)."""
    x64 = np.asarray(X, np.float64)
    q64 = np.asarray(onp.normalize_rows(Q) if metric == onp.METRIC_COS else Q, np.float64)
    out = np.empty((len(Q), len(X)))
    for b in range(len(Q)):
        if metric == onp.METRIC_L2:
            diff = x64 - q64[b]
            out[b] = np.einsum("nd,nd->n", diff, diff)
        else:
            out[b] = np.einsum("nd,d->n", x64, q64[b])
    return out


def ref_range(X, Q, radius, metric, id_offset=0):
    """(lims, D, I) of the definition: ascending ids, strict comparison with the float32 radius."""
    S = ref_scores(X, Q, metric) if len(X) else np.zeros((len(Q), 0))
    r = float(np.float32(radius))
    lims, D, I = [0], [], []
    for b in range(len(Q)):
        ids = np.nonzero(S[b] < r if metric == onp.METRIC_L2 else S[b] > r)[0]
        D.append(S[b, ids].astype(np.float32))
        I.append(ids.astype(np.int64) + id_offset)
        lims.append(lims[-1] + len(ids))
    return np.array(lims, np.int64), np.concatenate(D) if D else np.zeros(0, np.float32), \
        np.concatenate(I) if I else np.zeros(0, np.int64)


class RangeEngine:
    device = torch.device("cpu")

    def __init__(self, metric):
        self.metric, self.rows = metric, None

    @property
    def ntotal(self):
        return 0 if self.rows is None else len(self.rows)

    def add(self, x):
        x = np.asarray(x, np.float32)
        self.rows = x if self.rows is None else np.concatenate([self.rows, x])

    def range_search(self, q, radius, id_offset):
        rows = self.rows if self.rows is not None else np.zeros((0, np.asarray(q).shape[1]), np.float32)
        lims, D, I = ref_range(rows, np.asarray(q, np.float32), radius, self.metric, id_offset)
        return lims, torch.from_numpy(D), torch.from_numpy(I)


def _radius(X, Q, metric, per_query):
    S = ref_scores(X, Q, metric)
    k = min(per_query, S.shape[1])
    kth = np.sort(S, axis=1)[:, k - 1] if metric == onp.METRIC_L2 else -np.sort(-S, axis=1)[:, k - 1]
    return float(np.float32(np.median(kth)))


def _worker(rank, world, port, q_out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import probing_rag_amd as pra
        X = onp.synth_rows(42, 0, 301, 64)
        Q = onp.synth_rows(7, 0, 6, 64)
        res = {}
        for metric in (onp.METRIC_L2, onp.METRIC_IP, onp.METRIC_COS):
            for per_query in (0, 10, 200):
                ix = pra.ShardedFlatIndex(64, metric, engine=RangeEngine(metric))
                ix.add_global(X)                                  # ragged: 151 + 150 rows
                r = (-1.0 if metric == onp.METRIC_L2 else 1e30) if per_query == 0 else _radius(X, Q, metric, per_query)
                lims, D, I = ix.range_search(Q, r)
                res[(metric, per_query)] = (r, lims, D.numpy(), I.numpy())
        # uneven shards (rank 0: 17 rows, rank 1: the rest) and an empty shard (rank 0: none)
        for name, split in (("uneven", 17), ("empty", 0)):
            ix = pra.ShardedFlatIndex(64, onp.METRIC_L2, engine=RangeEngine(onp.METRIC_L2))
            if rank == 0 and split:
                ix.add_local(X[:split])
            if rank == 1:
                ix.add_local(X[split:])
            ix.sync()
            assert ix.id_offset == (0 if rank == 0 else split)
            r = _radius(X, Q, onp.METRIC_L2, 40)
            lims, D, I = ix.range_search(Q, r)
            res[name] = (r, lims, D.numpy(), I.numpy())
        q_out.put((rank, res))
    finally:
        dist.destroy_process_group()


def test_sharded_range_search_equals_unsharded_world2():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    ctx = mp.get_context("spawn")
    q_out = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q_out)) for r in range(2)]
    for p in procs:
        p.start()
    got = dict(q_out.get(timeout=120) for _ in range(2))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    X = onp.synth_rows(42, 0, 301, 64)
    Q = onp.synth_rows(7, 0, 6, 64)
    for key in got[0]:
        metric = onp.METRIC_L2 if key in ("uneven", "empty") else key[0]
        r = got[0][key][0]
        lims0, D0, I0 = ref_range(X, Q, r, metric)
        if key not in ("uneven", "empty") and key[1] == 0:
            assert lims0[-1] == 0
        else:
            assert lims0[-1] > len(Q)                     # something to compare
        for rank in (0, 1):
            _, lims, D, I = got[rank][key]
            assert np.array_equal(lims, lims0), key
            assert np.array_equal(I, I0), key
            assert np.array_equal(D, D0), key
            for b in range(len(Q)):
                seg = I[lims[b]:lims[b + 1]]
                assert np.all(np.diff(seg) > 0)           # ascending global ids, no sort needed
