"""CPU: faiss-style ID selectors (probing_rag_amd/selector.py) -> the word bitmap of a row window, for every selector
class and their composition, at windows that do and do not start on a multiple of 32."""
import numpy as np
import pytest

import probing_rag_amd as pra
from probing_rag_amd import selector as S

N_IDS = 4000
OFFSETS = (0, 1, 31, 33, 1000)


def _bitmap_bytes(member: np.ndarray) -> np.ndarray:
    """faiss's IDSelectorBitmap layout: id i -> bit (i & 7) of byte i >> 3."""
    out = np.zeros((len(member) + 7) // 8, np.uint8)
    for i in np.nonzero(member)[0]:
        out[i >> 3] |= np.uint8(1 << (i & 7))
    return out


def _cases():
    rng = np.random.default_rng(5)
    ids = np.arange(N_IDS)
    batch = rng.choice(N_IDS, 300, replace=False)
    bits = rng.random(N_IDS) < 0.3
    rng_sel = (37, 2900)
    cases = {
        "range": (S.IDSelectorRange(*rng_sel), (ids >= rng_sel[0]) & (ids < rng_sel[1])),
        "range_empty": (S.IDSelectorRange(50, 50), np.zeros(N_IDS, bool)),
        "batch": (S.IDSelectorBatch(batch), np.isin(ids, batch)),
        "array": (S.IDSelectorArray(list(batch[:17])), np.isin(ids, batch[:17])),
        "bitmap": (S.IDSelectorBitmap(_bitmap_bytes(bits)), bits),
        "bitmap_short": (S.IDSelectorBitmap(_bitmap_bytes(bits[:1500])), np.concatenate([bits[:1500], np.zeros(N_IDS - 1500, bool)])),
    }
    cases["not_batch"] = (S.IDSelectorNot(cases["batch"][0]), ~cases["batch"][1])
    cases["and"] = (S.IDSelectorAnd(cases["range"][0], cases["bitmap"][0]), cases["range"][1] & cases["bitmap"][1])
    cases["or"] = (S.IDSelectorOr(cases["batch"][0], cases["bitmap"][0]), cases["batch"][1] | cases["bitmap"][1])
    cases["nested"] = (S.IDSelectorAnd(S.IDSelectorNot(cases["or"][0]), cases["range"][0]),
                       ~cases["or"][1] & cases["range"][1])
    return cases


CASES = _cases()


@pytest.mark.parametrize("name", sorted(CASES))
@pytest.mark.parametrize("id0", OFFSETS)
def test_window_words_match_membership(name, id0):
    sel, member = CASES[name]
    for n in (0, 1, 31, 32, 33, 1000, N_IDS - id0):
        words = sel.window_words(id0, n)
        assert isinstance(words, np.ndarray) and words.dtype == np.uint32
        assert len(words) == (n + 31) // 32
        # bit (i & 31) of word (i >> 5) = local row i
        got = np.array([(int(words[i >> 5]) >> (i & 31)) & 1 for i in range(n)], bool)
        want = member[id0:id0 + n]
        assert np.array_equal(got, want), (name, id0, n)
        assert np.array_equal(sel.window_mask(id0, n), want)
    # is_member agrees with the window, also past the end of the id range
    probe = np.array([-1, 0, 5, 31, 32, N_IDS - 1, N_IDS, N_IDS + 77], np.int64)
    want = np.array([member[i] if 0 <= i < N_IDS else False for i in probe])
    if name.startswith("not") or name == "nested":
        want = None      # a complement selects ids outside [0, N_IDS) too
    if want is not None:
        assert np.array_equal(sel.is_member(probe), want), name


def test_bitmap_byte_layout_is_faiss():
    rng = np.random.default_rng(2)
    raw = rng.integers(0, 256, 97, dtype=np.uint8)
    sel = S.IDSelectorBitmap(raw)
    ids = np.arange(8 * len(raw) + 20)
    want = np.array([(raw[i >> 3] >> (i & 7)) & 1 if i < 8 * len(raw) else 0 for i in ids], bool)
    assert np.array_equal(sel.is_member(ids), want)
    for id0 in OFFSETS:
        n = 8 * len(raw) + 20 - id0
        assert np.array_equal(sel.window_mask(id0, n), want[id0:])
    # byte-aligned windows: the words ARE the bitmap's bytes, little-endian, padded to 4 B
    w = sel.window_words(0, 8 * len(raw))
    padded = np.zeros(4 * len(w), np.uint8)
    padded[:len(raw)] = raw
    assert np.array_equal(w.view(np.uint8), padded)
    # faiss's IDSelectorBitmap(n, bitmap): only the first ceil(n / 8) bytes count
    short = S.IDSelectorBitmap(raw, n=40)
    assert np.array_equal(short.is_member(ids), want & (ids < 40))


def test_search_parameters_and_exports():
    p = pra.SearchParameters(sel=pra.IDSelectorRange(3, 9))
    assert isinstance(p.sel, S.IDSelector)
    assert pra.SearchParameters().sel is None
    for name in ("IDSelectorRange", "IDSelectorBatch", "IDSelectorArray", "IDSelectorBitmap", "IDSelectorNot",
                 "IDSelectorAnd", "IDSelectorOr", "SearchParameters"):
        assert getattr(pra, name) is getattr(S, name)
