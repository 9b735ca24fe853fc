"""The ingest decoders on records whose expected columns are known by
construction (tests/ingest_cases.py): the Python twins in ops/ref.py and
ops/ref_l4.py and the HOST build of the kernel source (df_decode_*_host in
libdfcpu.so, the same l7_decode.h / l4_decode.h the GPU kernels compile)
must each give the expectation exactly -- well-formed edge cases, and
malformed records by the contract at the top of ops/csrc/l7_decode.h.
Then the pool and intern twins run on the same batches.
"""
import numpy as np
import pytest
import torch

import ingest_cases as IC
from deepflow_amd.ops import native, ref, ref_l4
from deepflow_amd.store import l7_schema as S


def decode(decoder: str, b: IC.Batch):
    seg = IC.make_segment(b.kind, b.n)
    sstr, sattr = IC.make_scratch(b.kind, b)
    if decoder == "ref":
        if b.kind == "l7":
            ref.decode_l7_ref(b.payload, b.offs, b.lens, seg, IC.BASE_ROW,
                              sstr, sattr)
        else:
            ref_l4.decode_l4_ref(b.payload, b.offs, b.lens, seg, IC.BASE_ROW,
                                 sstr)
        return seg, sstr, sattr
    lib = native.cpu()
    pay = IC.payload_tensor(b)
    assert pay.data_ptr() % 8 == 0
    offs, lens = torch.from_numpy(b.offs.copy()), torch.from_numpy(b.lens.copy())
    head = (pay.data_ptr(), offs.data_ptr(), lens.data_ptr(), b.n,
            seg.u64.data_ptr(), seg.u32.data_ptr(), seg.u8.data_ptr(),
            sstr.data_ptr())
    tail = (seg.capacity, IC.BASE_ROW, b.stride)
    if b.kind == "l7":
        rc = lib.df_decode_l7_host(*head, sattr.data_ptr(),
                                   seg.attr_cnt.data_ptr(), *tail)
    else:
        rc = lib.df_decode_l4_host(*head, *tail)
    assert rc == 0
    return seg, sstr, sattr


@pytest.fixture(scope="module", params=["l7", "l4"])
def kind(request):
    return request.param


def test_cases_cover_the_issue(kind):
    wf, mf = IC.cases(kind, False), [c for c in IC.cases(kind) if c.malformed]
    assert len({c.name for c in wf + mf}) == len(wf) + len(mf)
    assert len(wf) >= 15 and len(mf) >= 30
    for c in mf:    # a mutation loses something or at least changes bytes
        assert IC.build(c)[0] != IC.build(IC.Case("x", kind, IC.full(kind, 0)))[0]


@pytest.mark.parametrize("decoder", ["ref", "host"])
def test_every_case_alone(kind, decoder):
    """Each case as a one-record batch, so a failure names the case."""
    for c in IC.cases(kind):
        b = IC.make_batch(kind, [c])
        IC.check_decode(b, *decode(decoder, b))


@pytest.mark.parametrize("decoder", ["ref", "host"])
@pytest.mark.parametrize("n", IC.BATCH_SIZES)
def test_batches(kind, decoder, n):
    b = IC.batch(kind, n)
    assert b.n == n and len(b.payload) % 8 != 0 and b.stride > n
    for i, name in enumerate(b.names[:-1]):
        if "_lvl" in name or "_cut_" in name or "_len_" in name:
            assert b.names[i + 1].endswith("_follower")
    IC.check_decode(b, *decode(decoder, b))


def test_ref_and_host_agree_on_garbage(kind):
    """Neither decoder raises or leaves its record on arbitrary bytes, and
    they write the same thing (differential; the fuzz program covers the
    host build alone under a sanitizer)."""
    rng = np.random.default_rng(7)
    recs = [rng.integers(0, 256, int(rng.integers(0, 90)), dtype=np.uint8)
            .tobytes() for _ in range(200)]
    flips = []
    for c in IC.cases(kind, False):
        r = bytearray(IC.build(c)[0])
        if 0 < len(r) < 2000:
            for _ in range(4):
                r[int(rng.integers(0, len(r)))] = int(rng.integers(0, 256))
            flips.append(bytes(r))
    recs += flips
    payload = bytearray(b"\xff" * 3)
    offs, lens = [], []
    for r in recs:
        offs.append(len(payload))
        lens.append(len(r))
        payload += r
    b = IC.Batch(kind, ["g"] * len(recs), bytes(payload),
                 np.array(offs, dtype=np.uint32),
                 np.array(lens, dtype=np.uint32), [IC.Exp()] * len(recs))
    got = [decode(d, b) for d in ("ref", "host")]
    for (sa, ssa, saa), (sb, ssb, sab) in [got]:
        for x, y in ((sa.u64, sb.u64), (sa.u32, sb.u32), (sa.u8, sb.u8),
                     (ssa, ssb)):
            assert torch.equal(x, y)
        if kind == "l7":
            assert torch.equal(saa, sab)
            assert torch.equal(sa.attr_cnt, sb.attr_cnt)
    ss = got[0][1].numpy()
    for rid in range(b.n):
        for r in ss[:, rid]:
            if int(r) != IC.SENT_REF:
                off, ln = int(r) >> 16, int(r) & 0xFFFF
                assert offs[rid] <= off and off + ln <= offs[rid] + lens[rid]


@pytest.mark.parametrize("n", [1, 65, 257])
def test_pool_twins(kind, n):
    b = IC.batch(kind, n)
    seg, sstr, sattr = decode("ref", b)
    pc = IC.pool_cols(kind)
    row_len = ref.pool_lens_ref(sstr, pc, n)
    starts = torch.cumsum(row_len.to(torch.int64), 0) - row_len
    base, sent = 11, 0xEE
    seg.pool = torch.full((base + int(row_len.sum()) + 64,), sent,
                          dtype=torch.uint8)
    ref.pool_gather_ref(b.payload, seg, pc, IC.BASE_ROW, n, starts, base, sstr)
    IC.check_pool(b, row_len, seg.pool, base, sent, seg.str_lens,
                  seg.str_rowref)


@pytest.mark.parametrize("n", [1, 65, 257])
def test_intern_twins(n):
    b = IC.batch("l7", n)
    seg, sstr, sattr = decode("ref", b)
    tkeys = torch.zeros(1 << 12, dtype=torch.int64)
    rows = [sc for _, sc, _ in S.DID_COLS]
    doms = [d for _, _, d in S.DID_COLS]
    out = torch.full((S.N_DID, seg.capacity), 12345, dtype=torch.int32)
    new = ref.intern_ref(b.payload, sstr, rows, doms, 0, n, tkeys, out,
                         IC.BASE_ROW)
    new += ref.intern_attrs_pool_ref(b.payload, sattr, seg, IC.BASE_ROW, n,
                                     tkeys)
    by_slot = {(d, s): raw for d, s, raw in new}
    assert len(by_slot) == len(new), "one entry per (domain, string)"
    IC.check_ids(b, seg, out.numpy(), by_slot)
