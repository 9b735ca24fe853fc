"""GPU twins for the cold-segment codec: k_pack_bits/k_unpack_bits vs the
CPU reference packer (byte-identical words), and query-over-cold on the
GPU store."""
import pytest
import torch

from deepflow_amd.gen import SpanGenConfig
from deepflow_amd.gen.spans import gen_span_payload
from deepflow_amd.store import coldstore as C

pytestmark = pytest.mark.gpu

CFG = SpanGenConfig(n=2000, seed=33, tag_cardinality=50, n_attrs=2,
                    n_ips=64, n_services=4, n_resources=12)


def test_pack_kernel_matches_cpu():
    torch.manual_seed(7)
    for bits in (1, 5, 11, 17, 23, 32):
        hi = (1 << bits) - 1
        vals = torch.randint(0, min(hi + 1, 2**31), (4097,),
                             dtype=torch.int64)
        v32 = vals.to(torch.int32)
        want = C.pack_stream(v32, 0, bits)                       # CPU
        got = C.pack_stream(v32.cuda(), 0, bits)                 # kernel
        torch.cuda.synchronize()
        assert torch.equal(got.cpu(), want), bits
        back = C.unpack_stream(got, 4097, 0, bits)
        torch.cuda.synchronize()
        assert torch.equal(back.cpu(), v32), bits


def test_query_over_cold_gpu():
    from deepflow_amd.ingest import L7IngestPipeline
    from deepflow_amd.query.engine import QueryEngine
    pipe = L7IngestPipeline(device="cuda", segment_rows=1 << 11,
                            dict_capacity=1 << 12,
                            time_base_s=CFG.base_time_ns // 10**9)
    pipe.ingest_frame_payload(gen_span_payload(CFG))
    pipe.ingest_frame_payload(gen_span_payload(CFG))
    eng = QueryEngine(pipe, device="cuda")
    queries = [
        "SELECT Count(*) AS c FROM l7_flow_log",
        "SELECT l7_protocol, Count(*) AS c, Avg(response_duration) AS a "
        "FROM l7_flow_log GROUP BY l7_protocol ORDER BY c DESC",
    ]
    want = [eng.query(q) for q in queries]
    seg = pipe.segments.segments[0]
    hot_bytes = seg.stored_bytes_per_row() * seg.n_rows
    assert pipe.segments.demote_oldest()
    cold_bytes = pipe.segments.cold[0].compressed_bytes()
    assert hot_bytes / cold_bytes > 1.5
    got = [eng.query(q) for q in queries]
    assert want == got


def pack_bits_py(deltas, bits):
    """Bit-string packer: value i owns stream bits [i*bits, (i+1)*bits),
    least significant first; stream bit j is bit j%32 of word j//32."""
    s = "".join(format(d, f"0{bits}b")[::-1] for d in deltas)
    s += "0" * (-len(s) % 32)
    return [int(s[i:i + 32][::-1], 2) for i in range(0, len(s), 32)]


def _as_i32(vals):
    return torch.tensor([v - (1 << 32) if v >= (1 << 31) else v
                         for v in vals], dtype=torch.int32)


@pytest.mark.parametrize("base", [0, 12345, 2**31 + 7])
def test_pack_kernels_every_width(base):
    """Every width 1..32 at sizes around the 32-value period and past one
    block, values on both sides of the int32 sign bit."""
    import random
    rng = random.Random(base)
    for bits in range(1, 33):
        top = (1 << bits) - 1
        for n in (1, 31, 32, 33, 4097):
            deltas = [rng.randint(0, top) for _ in range(n)]
            deltas[0] = top
            deltas[-1] = top if n < 32 else 0
            deltas[n // 2] = top
            v32 = _as_i32([(base + d) & 0xFFFFFFFF for d in deltas])
            want = _as_i32(pack_bits_py(deltas, bits))
            got = C.pack_stream(v32.cuda(), base, bits)
            back = C.unpack_stream(got, n, base, bits)
            torch.cuda.synchronize()
            assert torch.equal(got.cpu(), want), (bits, n)
            assert torch.equal(back.cpu(), v32), (bits, n)


def test_constant_columns_pack_to_nothing():
    """A constant column (and an empty one) is (base, bits=0, no payload):
    neither kernel is launched for it."""
    n = 300
    m32 = torch.zeros((4, 512), dtype=torch.int32)
    m32[0, :n] = 7
    m32[1, :n] = -1                          # stored as 0xFFFFFFFF
    # columns are stored unsigned: 2^31-150 .. 2^31+149 is one 9-bit range
    m32[2, :n] = _as_i32([2**31 - 150 + i for i in range(n)])
    m32[3, :n] = -(2**31)
    m64 = torch.zeros((2, 512), dtype=torch.int64)
    m64[0, :n] = 2**40 + 3
    m64[1, :n] = 2**40 + torch.arange(n)
    for mat, const_rows in ((m32, {0, 1, 3}), (m64, {0})):
        dmat = mat.cuda()
        for rows in (n, 0):
            cols = C._compress_i32_matrix(dmat, rows)
            for c, pc in enumerate(cols):
                if rows == 0 or c in const_rows:
                    assert (pc.bits, pc.data, pc.raw) == (0, None, None)
                    assert pc.nbytes() == 0
                else:
                    assert pc.bits == 9 and pc.data.numel() == (n * 9 + 31) // 32
            out = torch.full_like(dmat, 99)
            C._restore_i32_matrix(cols, out, rows)
            torch.cuda.synchronize()
            assert torch.equal(out[:, :rows].cpu(), mat[:, :rows])
            assert bool((out[:, rows:] == 99).all())
