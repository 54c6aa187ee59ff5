"""faiss-style ID selectors for ``HipFlatIndex.search(x, k, params=SearchParameters(sel=...))``.

Same names and membership semantics as faiss (``faiss.SearchParameters``, ``faiss.IDSelectorRange`` / ``Batch`` /
``Array`` / ``Bitmap`` / ``Not`` / ``And`` / ``Or``).  Ids are in the id space ``search`` returns: row + id_offset (faiss's
own ids at offset 0).  Every selector turns itself into the word bitmap the library takes for a window of rows
``[id0, id0 + n)`` (``window_words``): uint32 words, bit ``i & 31`` of word ``i >> 5`` = local row i selected.  A
selector holding a CUDA bitmap produces its words on that device (no host round trip); all others produce NumPy arrays.
Importable without a GPU.
"""
import numpy as np

__all__ = ["SearchParameters", "IDSelector", "IDSelectorRange", "IDSelectorBatch", "IDSelectorArray", "IDSelectorBitmap",
           "IDSelectorNot", "IDSelectorAnd", "IDSelectorOr", "words_to_mask"]


def _n_words(n: int) -> int:
    return (int(n) + 31) // 32


def _pack_mask(mask: np.ndarray) -> np.ndarray:
    """bool [n] -> uint32 [ceil(n / 32)] (bit i & 31 of word i >> 5)."""
    n = len(mask)
    padded = np.zeros(_n_words(n) * 32, np.uint8)
    padded[:n] = mask
    return np.packbits(padded, bitorder="little").view("<u4").astype(np.uint32)


def words_to_mask(words, n: int) -> np.ndarray:
    """uint32 word bitmap (NumPy or CUDA) -> bool [n] on the host."""
    if not isinstance(words, np.ndarray):
        words = words.cpu().numpy()
    w = np.ascontiguousarray(words).astype("<u4", copy=False)
    return np.unpackbits(w.view(np.uint8), bitorder="little")[:int(n)].astype(bool)


class IDSelector:
    """Base class: ``is_member(ids)`` (bool array) and ``window_words(id0, n)`` (the library's bitmap)."""

    def is_member(self, ids) -> np.ndarray:
        return self._members(np.asarray(ids, np.int64))

    def _members(self, ids: np.ndarray) -> np.ndarray:
        raise NotImplementedError

    def _mask(self, id0: int, n: int) -> np.ndarray:
        return self._members(np.arange(int(id0), int(id0) + int(n), dtype=np.int64))

    def window_words(self, id0: int, n: int, device=None):
        """uint32 words of rows [id0, id0 + n): a NumPy array, or an int32 CUDA tensor with the same bits when the
        selector holds a CUDA bitmap (``device`` then names the GPU the words must be on)."""
        return _pack_mask(self._mask(int(id0), int(n)))

    def window_mask(self, id0: int, n: int) -> np.ndarray:
        """bool [n]: which of the rows [id0, id0 + n) are selected (host)."""
        return words_to_mask(self.window_words(id0, n), n)

    @property
    def is_cuda(self) -> bool:
        return False


class IDSelectorRange(IDSelector):
    """imin <= id < imax."""

    def __init__(self, imin: int, imax: int):
        self.imin, self.imax = int(imin), int(imax)

    def _members(self, ids):
        return (ids >= self.imin) & (ids < self.imax)

    def _mask(self, id0, n):
        m = np.zeros(n, bool)
        lo, hi = max(0, self.imin - id0), min(n, self.imax - id0)
        if hi > lo:
            m[lo:hi] = True
        return m


class IDSelectorArray(IDSelector):
    """id in ids (faiss IDSelectorArray: a plain list; IDSelectorBatch: the same set behind a hash)."""

    def __init__(self, ids):
        self.ids = np.unique(np.asarray(ids, np.int64).ravel())

    def _members(self, ids):
        return np.isin(ids, self.ids)

    def _mask(self, id0, n):
        m = np.zeros(n, bool)
        local = self.ids[(self.ids >= id0) & (self.ids < id0 + n)] - id0
        m[local] = True
        return m


class IDSelectorBatch(IDSelectorArray):
    pass


class IDSelectorBitmap(IDSelector):
    """faiss's byte layout: id i is selected iff i < 8 * len(bitmap) and (bitmap[i >> 3] >> (i & 7)) & 1.
    ``bitmap``: a NumPy uint8 array, or a CUDA uint8 tensor (kept on its device)."""

    def __init__(self, bitmap, n: int = None):
        if hasattr(bitmap, "is_cuda") and bitmap.is_cuda:
            import torch
            if bitmap.dtype != torch.uint8:
                raise ValueError("IDSelectorBitmap: expected a uint8 tensor")
            self.bitmap = bitmap.reshape(-1).contiguous()
        else:
            if hasattr(bitmap, "numpy"):
                bitmap = bitmap.numpy()
            self.bitmap = np.ascontiguousarray(bitmap, dtype=np.uint8).ravel()
        # (faiss's IDSelectorBitmap(n, bitmap) reads ceil(n / 8) bytes; ids past 8 * len are never selected)
        if n is not None:
            self.bitmap = self.bitmap[:(int(n) + 7) // 8]

    @property
    def is_cuda(self) -> bool:
        return not isinstance(self.bitmap, np.ndarray)

    def _host_bytes(self) -> np.ndarray:
        return self.bitmap if isinstance(self.bitmap, np.ndarray) else self.bitmap.cpu().numpy()

    def _members(self, ids):
        b = self._host_bytes()
        ok = (ids >= 0) & (ids < 8 * len(b))
        out = np.zeros(ids.shape, bool)
        i = ids[ok]
        out[ok] = ((b[i >> 3] >> (i & 7)) & 1).astype(bool)
        return out

    def _mask(self, id0, n):
        return self._members(np.arange(id0, id0 + n, dtype=np.int64))

    def window_words(self, id0: int, n: int, device=None):
        if not self.is_cuda:
            return super().window_words(id0, n)
        return _cuda_window_words(self.bitmap, int(id0), int(n))


def _cuda_window_words(bitmap, id0: int, n: int):
    """Bits [id0, id0 + n) of a CUDA byte bitmap as int32 words on its device (bits past the bitmap: clear)."""
    import torch
    nw = _n_words(n)
    dev = bitmap.device
    if n == 0:
        return torch.zeros(1, dtype=torch.int32, device=dev)
    if id0 >= 0 and id0 % 8 == 0:         # whole bytes: a slice, zero-padded to whole words
        b0 = id0 // 8
        src = bitmap[b0:b0 + 4 * nw]
        out = torch.zeros(4 * nw, dtype=torch.uint8, device=dev)
        out[:src.numel()] = src
        return out.view(torch.int32)
    # any other window: bits unpacked on the device, shifted, packed again
    ids = torch.arange(id0, id0 + 32 * nw, device=dev, dtype=torch.int64)
    ok = (ids >= 0) & (ids < 8 * bitmap.numel()) & (ids < id0 + n)
    ic = torch.where(ok, ids, torch.zeros_like(ids))
    bits = ((bitmap[ic >> 3].to(torch.int64) >> (ic & 7)) & 1) * ok.to(torch.int64)
    w = (bits.view(nw, 32) << torch.arange(32, device=dev, dtype=torch.int64)).sum(dim=1)
    return torch.where(w >= 2 ** 31, w - 2 ** 32, w).to(torch.int32)


def _combine(a, b, op):
    """word-wise op of two windows; a CUDA operand makes the result a CUDA tensor"""
    if isinstance(a, np.ndarray) and isinstance(b, np.ndarray):
        return op(a, b)
    import torch
    dev = a.device if not isinstance(a, np.ndarray) else b.device
    ta = a if not isinstance(a, np.ndarray) else torch.from_numpy(a.view(np.int32)).to(dev)
    tb = b if not isinstance(b, np.ndarray) else torch.from_numpy(b.view(np.int32)).to(dev)
    return op(ta, tb)


class IDSelectorNot(IDSelector):
    def __init__(self, sel: IDSelector):
        self.sel = sel

    @property
    def is_cuda(self) -> bool:
        return self.sel.is_cuda

    def _members(self, ids):
        return ~self.sel.is_member(ids)

    def window_words(self, id0: int, n: int, device=None):
        return ~self.sel.window_words(id0, n, device)     # (bits past n are ignored)


class IDSelectorAnd(IDSelector):
    def __init__(self, lhs: IDSelector, rhs: IDSelector):
        self.lhs, self.rhs = lhs, rhs

    @property
    def is_cuda(self) -> bool:
        return self.lhs.is_cuda or self.rhs.is_cuda

    def _members(self, ids):
        return self.lhs.is_member(ids) & self.rhs.is_member(ids)

    def window_words(self, id0: int, n: int, device=None):
        return _combine(self.lhs.window_words(id0, n, device), self.rhs.window_words(id0, n, device), lambda x, y: x & y)


class IDSelectorOr(IDSelectorAnd):
    def _members(self, ids):
        return self.lhs.is_member(ids) | self.rhs.is_member(ids)

    def window_words(self, id0: int, n: int, device=None):
        return _combine(self.lhs.window_words(id0, n, device), self.rhs.window_words(id0, n, device), lambda x, y: x | y)


class SearchParameters:
    """faiss.SearchParameters(sel=...): the selector applies to every query of the call."""

    def __init__(self, sel: IDSelector = None):
        self.sel = sel
