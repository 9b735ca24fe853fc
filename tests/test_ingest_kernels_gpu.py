"""The ingest kernels (k_decode_l7, k_decode_l4, k_pool_lens, k_pool_gather,
k_intern_many, k_intern_attrs) called directly through gpu_ops, no pipeline
object, against expectations known by construction (tests/ingest_cases.py).
All comparisons are exact.

The malformed records of ingest_cases.py reach the GPU only here and only
through the bounded parser of l7_decode.h / l4_decode.h, which
test_ingest_cases_cpu.py and test_decode_host_fuzz.py prove on the host
first (same source, host build).
"""
import numpy as np
import pytest
import torch

import ingest_cases as IC
from deepflow_amd.store import l7_schema as S

pytestmark = pytest.mark.gpu

DEV = "cuda"
FILL = 12345


@pytest.fixture(scope="module")
def ops():
    from deepflow_amd.ops import gpu_ops
    return gpu_ops


def gpu_decode(ops, b: IC.Batch):
    """-> (seg, sstr, sattr, payload tensor) after k_decode on the batch.
    The payload carries 4 KiB of zero bytes after the last record."""
    seg = IC.make_segment(b.kind, b.n, DEV)
    sstr, sattr = IC.make_scratch(b.kind, b, DEV)
    pay = IC.payload_tensor(b, tail=4096, device=DEV)
    offs = torch.from_numpy(b.offs.view(np.int32).copy()).to(DEV)
    lens = torch.from_numpy(b.lens.view(np.int32).copy()).to(DEV)
    if b.kind == "l7":
        ops.decode_l7(pay, offs, lens, seg, IC.BASE_ROW, sstr, sattr)
    else:
        ops.decode_l4(pay, offs, lens, seg, IC.BASE_ROW, sstr)
    torch.cuda.synchronize()
    return seg, sstr, sattr, pay


@pytest.mark.parametrize("kind", ["l7", "l4"])
@pytest.mark.parametrize("n", IC.BATCH_SIZES)
def test_decode(ops, kind, n):
    b = IC.batch(kind, n)
    seg, sstr, sattr, _ = gpu_decode(ops, b)
    IC.check_decode(b, seg, sstr, sattr)


@pytest.mark.parametrize("kind", ["l7", "l4"])
@pytest.mark.parametrize("n", [1, 65, 257])
def test_pool(ops, kind, n):
    """Zero-length rows, 32767 / 32768 / 65535-byte strings and a row over
    65535 are all in the 257 batch; pool_base is non-zero."""
    b = IC.batch(kind, n)
    if n == 257 and kind == "l7":
        assert {"l7_empty", "l7_str_32767", "l7_str_32768", "l7_str_65535",
                "l7_row_pool_over_64k"} <= set(b.names)
    seg, sstr, _, pay = gpu_decode(ops, b)
    pc = torch.tensor(IC.pool_cols(kind), dtype=torch.uint8, device=DEV)
    row_len = torch.full((n + 3,), FILL, dtype=torch.int32, device=DEV)
    ops.pool_lens(sstr, pc, n, row_len)
    torch.cuda.synchronize()
    assert (row_len[n:] == FILL).all()
    rl = row_len[:n].to(torch.int64)
    starts = torch.cumsum(rl, 0) - rl
    base, sent = 11, 0xEE
    pool = torch.full((base + int(rl.sum()) + 64,), sent, dtype=torch.uint8,
                      device=DEV)
    ops.pool_gather(pay, seg, pc, IC.BASE_ROW, n, starts, pool, base, sstr)
    torch.cuda.synchronize()
    IC.check_pool(b, row_len[:n], pool, base, sent, seg.str_lens,
                  seg.str_rowref)


# ------------------------------------------------------------- intern

class Strings:
    """A payload of strings and the refs into it."""

    def __init__(self):
        self.buf = bytearray(b"\xff" * 5)

    def ref(self, s: bytes) -> int:
        off = len(self.buf)
        self.buf += s
        return off << 16 | len(s)

    def tensor(self):
        t = torch.zeros((len(self.buf) + 7) // 8 * 8 + 64, dtype=torch.uint8)
        t[:len(self.buf)] = torch.frombuffer(self.buf, dtype=torch.uint8)
        return t.to(DEV)


class Table:
    def __init__(self, cap=1 << 10, emit_cap=1 << 10):
        self.tkeys = torch.zeros(cap, dtype=torch.int64, device=DEV)
        # one sentinel row after the emit buffer
        self.emit_all = torch.full((emit_cap + 1, 2), FILL, dtype=torch.int64,
                                   device=DEV)
        self.emit = self.emit_all[:emit_cap]
        self.ctr = torch.zeros(1, dtype=torch.int32, device=DEV)

    def entries(self, buf) -> dict:
        """(domain, slot) -> bytes, from the emit rows."""
        torch.cuda.synchronize()
        assert (self.emit_all[-1] == FILL).all(), "emit written past its cap"
        cnt = min(int(self.ctr.item()), self.emit.shape[0])
        out = {}
        for slot_w, ref in self.emit[:cnt].cpu().numpy().view(np.uint64).tolist():
            k = (slot_w >> 56, slot_w & 0xFFFFFFFF)
            assert k not in out, "slot emitted twice"
            out[k] = bytes(buf[ref >> 16:(ref >> 16) + (ref & 0xFFFF)])
        return out


def intern_cols(ops, cols, domains, tab: Table, n=None):
    """cols: per column a list of n byte strings (b"" = absent).
    -> (out_ids [C, n] numpy int64 of u32 ids, Strings)."""
    n = len(cols[0]) if n is None else n
    st = Strings()
    stride = n + 7
    refs = torch.zeros((len(cols), stride), dtype=torch.int64)
    for c, col in enumerate(cols):
        for i, s in enumerate(col):
            refs[c, i] = st.ref(s)
    out = torch.full((len(cols), n + 9), FILL, dtype=torch.int32, device=DEV)
    ops.intern_many(st.tensor(), refs.to(DEV),
                    torch.arange(len(cols), dtype=torch.int16, device=DEV),
                    torch.tensor(domains, dtype=torch.uint8, device=DEV),
                    0, n, tab.tkeys, tab.emit, tab.ctr, out, 4)
    torch.cuda.synchronize()
    o = out.cpu().numpy()
    assert (o[:, :4] == FILL).all() and (o[:, 4 + n:] == FILL).all()
    return o[:, 4:4 + n].astype(np.int64) & 0xFFFFFFFF, st


def check_hydrated(ids, cols, domains, entries):
    for c, col in enumerate(cols):
        for i, s in enumerate(col):
            if s:
                assert entries[(domains[c], int(ids[c, i]))] == s, (c, i)
            else:
                assert int(ids[c, i]) == S.DICT_ID_INVALID, (c, i)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 130])
def test_intern_many_two_columns(ops, n):
    """Two columns, so a wave straddles two domains; the same bytes in
    both domains get two entries; a second launch emits nothing."""
    cols = [[b"s%d" % (i % 7) for i in range(n)],
            [b"" if i % 5 == 0 else b"s%d" % (i % 3) for i in range(n)]]
    doms = [0, 1]
    tab = Table()
    ids, st = intern_cols(ops, cols, doms, tab)
    entries = tab.entries(st.buf)
    check_hydrated(ids, cols, doms, entries)
    want = {(d, s) for d, col in zip(doms, cols) for s in col if s}
    assert int(tab.ctr.item()) == len(want) == len(entries)
    assert {(d, s) for (d, _), s in entries.items()} == want
    tab.ctr.zero_()
    ids2, _ = intern_cols(ops, cols, doms, tab)
    assert int(tab.ctr.item()) == 0 and (ids2 == ids).all()


def test_intern_many_uniform_waves(ops):
    """One wave per column: every lane the same string, the same with lane
    0 empty, and all lanes empty."""
    cols = [[b"same"] * 64, [b""] + [b"same"] * 63, [b""] * 64]
    doms = [2, 2, 2]
    tab = Table()
    ids, st = intern_cols(ops, cols, doms, tab)
    entries = tab.entries(st.buf)
    check_hydrated(ids, cols, doms, entries)
    assert int(tab.ctr.item()) == 1


def test_intern_many_emit_cap(ops):
    n, cap = 100, 10
    cols = [[b"str-%03d" % i for i in range(n)]]
    tab = Table(emit_cap=cap)
    ids, st = intern_cols(ops, cols, [3], tab)
    torch.cuda.synchronize()
    assert int(tab.ctr.item()) == n, "emit_ctr reports the true count"
    entries = tab.entries(st.buf)       # also checks the row after the cap
    assert len(entries) == cap
    assert len(set(ids[0].tolist())) == n and \
        S.DICT_ID_INVALID not in ids[0].tolist()


def test_intern_many_full_table(ops):
    n, cap = 100, 64
    cols = [[b"distinct-%03d" % i for i in range(n)]]
    tab = Table(cap=cap)
    ids, st = intern_cols(ops, cols, [4], tab)
    invalid = int((ids[0] == S.DICT_ID_INVALID).sum())
    assert invalid == n - cap
    entries = tab.entries(st.buf)
    assert len(entries) == cap
    for i, s in enumerate(cols[0]):
        if ids[0, i] != S.DICT_ID_INVALID:
            assert entries[(4, int(ids[0, i]))] == s


@pytest.mark.parametrize("n", [1, 65, 257])
def test_intern_on_decoded_batches(ops, n):
    """decode -> intern_many + intern_attrs on the case batches: ids
    hydrate to the expected strings, attr_pool has the expected layout."""
    b = IC.batch("l7", n)
    seg, sstr, sattr, pay = gpu_decode(ops, b)
    tab = Table(cap=1 << 12, emit_cap=1 << 12)
    seg.did.fill_(FILL)
    ops.intern_many(pay, sstr,
                    torch.tensor([sc for _, sc, _ in S.DID_COLS],
                                 dtype=torch.int16, device=DEV),
                    torch.tensor([d for _, _, d in S.DID_COLS],
                                 dtype=torch.uint8, device=DEV),
                    0, n, tab.tkeys, tab.emit, tab.ctr, seg.did, IC.BASE_ROW)
    cnt = seg.attr_cnt[IC.BASE_ROW:IC.BASE_ROW + n].to(torch.int32)
    starts = (torch.cumsum(2 * cnt, 0) - 2 * cnt).to(torch.int32)
    seg.attr_start[IC.BASE_ROW:IC.BASE_ROW + n] = starts
    seg.attr_pool = torch.full((2 * S.MAX_ATTRS * n + 8,), FILL,
                               dtype=torch.int32, device=DEV)
    ops.intern_attrs(pay, seg, IC.BASE_ROW, n, tab.tkeys, tab.emit, tab.ctr,
                     sattr, starts)
    entries = tab.entries(b.payload)
    IC.check_ids(b, seg, seg.did.cpu().numpy(), entries, FILL)
    used = int((2 * cnt).sum())
    assert (seg.attr_pool[used:] == FILL).all()


@pytest.mark.parametrize("n", [1, 63, 64, 65, 130])
@pytest.mark.parametrize("names", ["equal", "different"])
def test_intern_attrs_layout(ops, n, names):
    """Rows of count 0 and of count L7_MAX_ATTRS mixed in one wave, an empty
    name (-1) and an empty value; names at [start, start+cnt), values at
    [start+cnt, start+2*cnt), one sentinel slot around every row's block."""
    M = S.MAX_ATTRS
    st = Strings()
    seg = IC.make_segment("l7", n, DEV)
    stride = n + 7
    sattr = torch.full((2 * M, stride), IC.SENT_REF, dtype=torch.int64)
    cnts, want = [], []
    for i in range(n):
        c = (0, M, 3)[i % 3]
        row = []
        for a in range(c):
            nm = b"" if (i % 7 == 1 and a == 1) else \
                (b"name-%d" % a if names == "equal" else b"n-%d-%d" % (i, a))
            vl = b"" if (i % 5 == 1 and a == 0) else b"v-%d-%d" % (i % 11, a)
            sattr[a, i] = st.ref(nm)
            sattr[M + a, i] = st.ref(vl)
            row.append((nm, vl))
        cnts.append(c)
        want.append(row)
    cnt = torch.tensor(cnts, dtype=torch.int32)
    seg.attr_cnt[IC.BASE_ROW:IC.BASE_ROW + n] = cnt.to(torch.uint8).to(DEV)
    blk = 2 * cnt + 1                    # one sentinel slot after each block
    starts = (torch.cumsum(blk, 0) - blk + 1).to(torch.int32)
    total = int(blk.sum()) + 1
    seg.attr_pool = torch.full((total + 8,), FILL, dtype=torch.int32,
                               device=DEV)
    tab = Table(cap=1 << 12, emit_cap=1 << 12)
    ops.intern_attrs(st.tensor(), seg, IC.BASE_ROW, n, tab.tkeys, tab.emit,
                     tab.ctr, sattr.to(DEV), starts.to(DEV))
    entries = tab.entries(st.buf)
    pool = seg.attr_pool.cpu().numpy()
    touched = np.zeros(len(pool), dtype=bool)
    for i, row in enumerate(want):
        s, c = int(starts[i]), cnts[i]
        touched[s:s + 2 * c] = True
        for a, (nm, vl) in enumerate(row):
            for at, dom, s_ in ((s + a, S.DICT_DOM_ATTR_NAME, nm),
                                (s + c + a, S.DICT_DOM_ATTR_VALUE, vl)):
                if s_:
                    assert entries[(dom, int(pool[at]))] == s_, (i, a)
                else:
                    assert int(pool[at]) == -1, (i, a)
    assert (pool[~touched] == FILL).all(), "attr_pool written outside blocks"
    want_entries = {(S.DICT_DOM_ATTR_NAME, nm) for r in want for nm, _ in r if nm} \
        | {(S.DICT_DOM_ATTR_VALUE, vl) for r in want for _, vl in r if vl}
    assert {(d, s) for (d, _), s in entries.items()} == want_entries
    assert int(tab.ctr.item()) == len(want_entries)
