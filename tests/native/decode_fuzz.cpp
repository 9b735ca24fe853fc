// Stand-alone fuzz of the HOST build of the ingest decoders
// (ops/csrc/l7_decode.h, l4_decode.h -- the text k_decode_l7/l4 compile).
// Built by tests/test_decode_host_fuzz.py with
//   g++ -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all
// together with dfcpu.cpp (the span generator). AddressSanitizer is the
// bounds oracle: every mutated record is decoded ALONE in a fresh heap
// buffer of its length rounded up to 8, so a read past the record's word
// or a write past a column faults. Termination is the hang oracle. The
// program itself checks that every emitted string ref lies in [0, len).
//
// usage: decode_fuzz <flows.bin> <mutations per record and kind>
//   flows.bin: [u32 len][TaggedFlow bytes]* (gen/flows.py gen_flow_payload)
#define DF_HOST_BUILD 1
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "l7_decode.h"
#include "l4_decode.h"

struct SpanCfg {  // dfcpu.cpp SpanCfg
    uint64_t seed, base_time_ns, dt_ns;
    uint32_t n_agents, n_ips, n_epcs, n_services, n_resources,
        tag_cardinality, n_attrs, err_rate_pct, ip6_rate_pct;
};
extern "C" uint64_t df_gen_spans_indexed(const SpanCfg*, uint64_t, uint64_t,
                                         uint8_t*, uint64_t, uint32_t*,
                                         uint32_t*);
extern "C" uint64_t df_scan_offsets(const uint8_t*, uint64_t, uint32_t*,
                                    uint32_t*, uint64_t);

static const uint64_t SENT = 0x7FFFFFF0ull << 16;
static uint64_t lcg_state = 0x2545F4914F6CDD1Dull;
static uint32_t lcg() {
    lcg_state = lcg_state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(lcg_state >> 33);
}
static uint64_t n_decodes = 0;

static int check_refs(const uint64_t* refs, int n, uint32_t len,
                      const char* what) {
    for (int i = 0; i < n; i++) {
        if (refs[i] == SENT) continue;
        uint64_t off = STR_REF_OFF(refs[i]), ln = STR_REF_LEN(refs[i]);
        if (off + ln > len) {
            fprintf(stderr, "%s: ref %d [%llu,+%llu) leaves record of %u\n",
                    what, i, (unsigned long long)off, (unsigned long long)ln,
                    len);
            return 1;
        }
    }
    return 0;
}

// decode `len` bytes alone in a fresh heap block of len rounded up to 8
static int decode_one(bool l7, const uint8_t* rec, uint32_t len) {
    size_t cap = ((size_t)len + 7) & ~(size_t)7;
    uint8_t* buf = (uint8_t*)malloc(cap ? cap : 8);
    memcpy(buf, rec, len);
    memset(buf + len, 0xA5, cap - len);
    uint32_t off = 0;
    ByteStream bs;
    bs.init(buf);
    int bad;
    n_decodes++;
    if (l7) {
        std::vector<uint64_t> u64c(L7_U64_N), strc(L7_STR_N, SENT),
            attrc(2 * L7_MAX_ATTRS, SENT);
        std::vector<uint32_t> u32c(L7_U32_N);
        std::vector<uint8_t> u8c(L7_U8_N), cnt(1, 0xEE);
        L7Cols cols{u64c.data(), u32c.data(), u8c.data(), strc.data(),
                    attrc.data(), cnt.data(), 1, 0, 1};
        decode_l7_record(bs, off, len, 0, cols);
        bad = check_refs(strc.data(), L7_STR_N, len, "l7 str") |
              check_refs(attrc.data(), 2 * L7_MAX_ATTRS, len, "l7 attr");
        if (cnt[0] > L7_MAX_ATTRS) {
            fprintf(stderr, "attr_cnt %u not written\n", cnt[0]);
            bad = 1;
        }
    } else {
        std::vector<uint64_t> u64c(L4_U64_N), strc(L4_STR_N, SENT);
        std::vector<uint32_t> u32c(L4_U32_N);
        std::vector<uint8_t> u8c(L4_U8_N);
        L4Cols cols{u64c.data(), u32c.data(), u8c.data(), strc.data(), 1, 0, 1};
        decode_l4_record(bs, off, len, 0, cols);
        bad = check_refs(strc.data(), L4_STR_N, len, "l4 str");
    }
    free(buf);
    return bad;
}

// positions of the length bytes of the length-delimited fields, walking
// `depth` message levels (every such field is tried as a sub-message)
static void len_bytes(const uint8_t* p, uint32_t pos, uint32_t end, int depth,
                      std::vector<uint32_t>& out) {
    auto rd = [&](uint64_t& v) {
        v = 0;
        for (int sh = 0; sh < 64 && pos < end; sh += 7) {
            uint8_t b = p[pos++];
            v |= (uint64_t)(b & 0x7F) << sh;
            if (!(b & 0x80)) return true;
        }
        return false;
    };
    while (pos < end) {
        uint64_t k, v;
        if (!rd(k)) return;
        switch (k & 7) {
            case 0: if (!rd(v)) return; break;
            case 1: pos += 8; break;
            case 5: pos += 4; break;
            case 2: {
                uint32_t at = pos;
                if (!rd(v) || v > end - pos) return;
                out.push_back(at);
                if (depth > 1)
                    len_bytes(p, pos, pos + (uint32_t)v, depth - 1, out);
                pos += (uint32_t)v;
                break;
            }
            default: return;
        }
    }
}

static int fuzz_record(bool l7, const uint8_t* rec, uint32_t len, int muts) {
    int bad = decode_one(l7, rec, len);
    for (uint32_t cut = 0; cut < len; cut++)     // truncate at every length
        bad |= decode_one(l7, rec, cut);
    std::vector<uint8_t> m(rec, rec + len);
    std::vector<uint32_t> lb;
    len_bytes(rec, 0, len, 5, lb);
    for (int i = 0; i < muts && len; i++) {
        uint32_t at = lcg() % len;               // flip one byte
        uint8_t keep = m[at];
        m[at] ^= (uint8_t)(1u << (lcg() & 7));
        bad |= decode_one(l7, m.data(), len);
        m[at] = 0xFF;                            // overwrite with 0xFF
        bad |= decode_one(l7, m.data(), len);
        m[at] = keep;
        if (!lb.empty()) {                       // length byte -> 0x80..0xFF
            at = lb[lcg() % lb.size()];
            keep = m[at];
            m[at] = (uint8_t)(0x80 | (lcg() & 0x7F));
            bad |= decode_one(l7, m.data(), len);
            m[at] = keep;
        }
    }
    return bad;
}

int main(int argc, char** argv) {
    if (argc < 3) {
        fprintf(stderr, "usage: decode_fuzz flows.bin mutations\n");
        return 2;
    }
    int muts = atoi(argv[2]);
    const uint32_t N = 256;
    int bad = 0;

    SpanCfg cfg{9, 1700000000000000000ull, 1000, 4, 128, 4, 16, 64, 200, 4,
                5, 20};
    std::vector<uint32_t> offs(N), lens(N);
    uint64_t need = df_gen_spans_indexed(&cfg, 0, N, nullptr, 0, nullptr, nullptr);
    std::vector<uint8_t> spans(need);
    df_gen_spans_indexed(&cfg, 0, N, spans.data(), need, offs.data(), lens.data());
    for (uint32_t i = 0; i < N; i++)
        bad |= fuzz_record(true, spans.data() + offs[i], lens[i], muts);

    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    std::vector<uint8_t> flows;
    uint8_t chunk[65536];
    for (size_t n; (n = fread(chunk, 1, sizeof chunk, f)) > 0;)
        flows.insert(flows.end(), chunk, chunk + n);
    fclose(f);
    uint64_t nf = df_scan_offsets(flows.data(), flows.size(), offs.data(),
                                  lens.data(), N);
    if (nf != N) {
        fprintf(stderr, "expected %u flows, found %llu\n", N,
                (unsigned long long)nf);
        return 2;
    }
    for (uint32_t i = 0; i < N; i++)
        bad |= fuzz_record(false, flows.data() + offs[i], lens[i], muts);

    printf("decode_fuzz: %llu decodes, %s\n", (unsigned long long)n_decodes,
           bad ? "REFS OUT OF RANGE" : "ok");
    return bad ? 1 : 0;
}
