"""numpy statement of the Elias-Fano id map of an inverted file (include/pqh.h, "compressed
ids"), written from the format alone: python integers row by row, no
word tricks.  With B = the bit width of n_ids - 1 and key(s) = (list(s) << B) | perm[s]:

    header   16 u64 words: magic, n, n_ids, nlist, B, L, low offset, high offset, high words,
             sample offset, samples, reverse offset, bytes of a reverse entry (0: none), words
             of the blob, two zeros -- offsets in words from the start of the blob
    low      n fields of L bits, field s at bit s * L, L = max(0, floor(log2((nlist << B) / n)))
    high     bit (key(s) >> L) + s set for every row s; ((nlist << B) - 1 >> L) + n bits
    samples  one word per 256 rows: the high-bit position of row 256 j
    reverse  the list of every id: u16 (0xFFFF: none) where nlist <= 65535, else int32 (-1: none)

Every part is padded to whole words with zeros."""
import numpy as np

HDR_WORDS = 16
MAGIC = int.from_bytes(b"PQIDMAP1", "little")


def shape(n, n_ids, nlist, reverse=True):
    """every derived number of the format, as a dict"""
    assert 0 <= n <= n_ids < 2 ** 31 and 1 <= nlist <= 2 ** 24
    B = (n_ids - 1).bit_length() if n_ids > 0 else 0
    universe = nlist << B
    L = max(0, (universe // n).bit_length() - 1) if n > 0 else 0
    rev_size = 0 if not reverse else 2 if nlist <= 65535 else 4
    high_bits = (((universe - 1) >> L) + n) if n > 0 else 0
    s = dict(n=n, n_ids=n_ids, nlist=nlist, B=B, L=L, rev_size=rev_size, high_bits=high_bits)
    s["low"] = HDR_WORDS
    s["low_words"] = (n * L + 63) // 64
    s["high"] = s["low"] + s["low_words"]
    s["high_words"] = (high_bits + 63) // 64
    s["samp"] = s["high"] + s["high_words"]
    s["samps"] = (n + 255) // 256
    s["rev"] = s["samp"] + s["samps"]
    s["rev_words"] = (n_ids * rev_size + 7) // 8
    s["words"] = s["rev"] + s["rev_words"]
    return s


def idmap_bytes(n, n_ids, nlist, reverse=True):
    return shape(n, n_ids, nlist, reverse)["words"] * 8


def lists_of(offsets, n):
    """the list of every stream row"""
    offsets = np.asarray(offsets, np.int64)
    assert offsets[0] == 0 and offsets[-1] == n and (np.diff(offsets) >= 0).all()
    return np.repeat(np.arange(len(offsets) - 1, dtype=np.int64), np.diff(offsets))


def keys_of(perm, offsets, n_ids):
    perm = np.asarray(perm, np.int64)
    B = (n_ids - 1).bit_length() if n_ids > 0 else 0
    return [(int(l) << B) | int(p) for l, p in zip(lists_of(offsets, len(perm)), perm)]


def build(perm, offsets, n_ids, reverse=True):
    """the blob, as a uint8 array"""
    perm = np.asarray(perm, np.int64)
    n, nlist = len(perm), len(offsets) - 1
    s = shape(n, n_ids, nlist, reverse)
    keys = keys_of(perm, offsets, n_ids)
    assert all(0 <= p < n_ids for p in perm.tolist())
    assert all(a < b for a, b in zip(keys, keys[1:])), "the ids of a list must ascend"
    L = s["L"]
    low = high = 0          # each part as one python integer, bit 0 first
    samples = []
    for r, key in enumerate(keys):
        low |= (key & ((1 << L) - 1)) << (r * L)
        pos = (key >> L) + r
        assert pos < s["high_bits"]
        high |= 1 << pos
        if r % 256 == 0:
            samples.append(pos)
    header = [MAGIC, n, n_ids, nlist, s["B"], L, s["low"], s["high"], s["high_words"], s["samp"],
              s["samps"], s["rev"], s["rev_size"], s["words"], 0, 0]
    blob = np.array(header, dtype="<u8").tobytes()
    blob += low.to_bytes(s["low_words"] * 8, "little")
    blob += high.to_bytes(s["high_words"] * 8, "little")
    blob += np.array(samples, dtype="<u8").tobytes()
    if s["rev_size"]:
        dtype, none = ("<u2", 0xFFFF) if s["rev_size"] == 2 else ("<i4", -1)
        rev = np.full(n_ids, none, dtype=dtype)
        rev[perm] = lists_of(offsets, n).astype(dtype)
        rev = rev.tobytes()
        blob += rev + bytes(s["rev_words"] * 8 - len(rev))
    assert len(blob) == s["words"] * 8
    return np.frombuffer(blob, dtype=np.uint8).copy()


class View:
    """a blob read back, every part as python integers"""

    def __init__(self, blob):
        w = np.frombuffer(np.asarray(blob, np.uint8).tobytes(), dtype="<u8")
        h = [int(v) for v in w[:HDR_WORDS]]
        assert h[0] == MAGIC and h[14] == 0 and h[15] == 0 and h[13] == len(w)
        (self.n, self.n_ids, self.nlist, self.B, self.L, low, high, self.high_words, samp, samps,
         rev, self.rev_size) = h[1:13]
        self.low = int.from_bytes(w[low:high].tobytes(), "little")
        self.high = np.unpackbits(np.frombuffer(w[high:samp].tobytes(), np.uint8), bitorder="little")
        self.samples = [int(v) for v in w[samp:samp + samps]]
        self.rev = None
        if self.rev_size:
            raw = w[rev:].tobytes()[:self.n_ids * self.rev_size]
            self.rev = np.frombuffer(raw, dtype="<u2" if self.rev_size == 2 else "<i4").astype(np.int64)
            if self.rev_size == 2:
                self.rev[self.rev == 0xFFFF] = -1

    def key(self, r):
        """select: the sample of the row's block, then set bits counted up to the row's"""
        assert 0 <= r < self.n
        start = self.samples[r >> 8]
        assert self.high[start] == 1                      # the sample is the block's first row
        pos = start + int(np.flatnonzero(self.high[start:])[r & 255])
        return ((pos - r) << self.L) | ((self.low >> (r * self.L)) & ((1 << self.L) - 1))

    def id(self, r):
        return self.key(r) & ((1 << self.B) - 1)


def ids(blob, rows):
    """ids of stream rows; a negative row is copied through, a row >= n gives -1"""
    v = View(blob)
    rows = np.asarray(rows, np.int64)
    out = [r if r < 0 else v.id(r) if r < v.n else -1 for r in rows.ravel().tolist()]
    return np.array(out, np.int64).reshape(rows.shape)


def decode(blob, first=0, count=None):
    v = View(blob)
    count = v.n - first if count is None else count
    assert 0 <= first and 0 <= count and first + count <= v.n
    return np.array([v.id(r) for r in range(first, first + count)], np.int64)


def rows(blob, offsets, want):
    """stream rows of ids: the list from the reverse part, a binary search of its rows by key;
    -1 for an id without a row or outside [0, n_ids)"""
    v = View(blob)
    assert v.rev is not None
    out = []
    for i in np.asarray(want, np.int64).ravel().tolist():
        row = -1
        if 0 <= i < v.n_ids and v.rev[i] >= 0:
            l = int(v.rev[i])
            lo, hi = int(offsets[l]), int(offsets[l + 1])
            key = (l << v.B) | i
            while lo < hi:
                mid = (lo + hi) // 2
                if v.key(mid) < key:
                    lo = mid + 1
                else:
                    hi = mid
            if lo < int(offsets[l + 1]) and v.key(lo) == key:
                row = lo
        out.append(row)
    return np.array(out, np.int64).reshape(np.asarray(want).shape)


def pack_mask(blob, keep):
    """uint32 words: bit s & 31 of word s >> 5 = keep[id(s)]"""
    v = View(blob)
    words = np.zeros((v.n + 31) // 32, np.uint32)
    for r in range(v.n):
        if keep[v.id(r)]:
            words[r >> 5] |= np.uint32(1 << (r & 31))
    return words


def decode_span_words(blob, j):
    """the high-bit words block j of 256 rows spans, from its sample to its last row's bit"""
    v = View(blob)
    last = min(256 * j + 255, v.n - 1)
    key = v.key(last)
    return (((key >> v.L) + last) >> 6) - (v.samples[j] >> 6) + 1


# ---- the shapes of the tests: (perm, offsets, n_ids) --------------------------------------
def random_layout(n, n_ids, nlist, seed, empty=()):
    """n distinct ids of [0, n_ids) spread over the lists not named in `empty`, ascending
    inside every list: what IVF.build, add and compact leave behind"""
    rng = np.random.default_rng(seed)
    chosen = rng.choice(n_ids, n, replace=False) if n_ids < (1 << 24) else \
        np.unique(rng.integers(0, n_ids, 4 * n + 8))[:n]
    assert len(chosen) == n
    usable = np.array([l for l in range(nlist) if l not in empty], np.int64)
    lists = usable[rng.integers(0, len(usable), n)] if nlist <= (1 << 16) else \
        rng.integers(0, nlist, n).astype(np.int64)
    order = np.lexsort((chosen, lists))
    perm = np.asarray(chosen, np.int64)[order]
    offsets = np.zeros(nlist + 1, np.int64)
    np.cumsum(np.bincount(lists, minlength=nlist), out=offsets[1:])
    return perm, offsets, n_ids


def two_ends(nlist=1024, per=150, last=None):
    """only the first (per rows) and the last list (`last` rows, default per) populated: a gap
    in the keys inside block 0.  The high part has fewer than 3 n + 1 bits, so the gap spans
    more than 64 words only from some 2,100 rows on: last=4000 is that case."""
    last = per if last is None else last
    n = per + last
    ids = np.random.default_rng(n).permutation(n)
    perm = np.concatenate([np.sort(ids[:per]), np.sort(ids[per:])]).astype(np.int64)
    offsets = np.full(nlist + 1, per, np.int64)
    offsets[0], offsets[-1] = 0, n
    return perm, offsets, n


def last_list(n=300, nlist=1024):
    offsets = np.zeros(nlist + 1, np.int64)
    offsets[-1] = n
    return np.arange(n, dtype=np.int64), offsets, n


def identity(n):
    return np.arange(n, dtype=np.int64), np.array([0, n], np.int64), n
