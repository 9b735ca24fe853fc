// Column layout ABI for decoded L7 flow logs (spans).
//
// The decode kernel (K1) writes straight into columnar segment slices laid
// out as one tensor per width class: u64 [L7_U64_N, stride], u32
// [L7_U32_N, stride], u8 [L7_U8_N, stride], and string-reference u64 columns
// [L7_STR_N, stride] packed as (byte_offset << 16 | min(len, 0xFFFF)).
// Mirrored in deepflow_amd/store/l7_schema.py — keep in sync (test:
// tests/test_layout_sync.py).
//
// Column set models the reference ClickHouse l7_flow_log schema
// (server/ingester/flow_log/log_data/l7_flow_log.go:101-283) minus
// CH-specific materialization; KnowledgeGraph columns are produced by the
// tag-join kernel (K2) into the kg block.
#pragma once
#include <stdint.h>

// ---- u64 columns ----
enum {
    L7_U64_START_TIME = 0,  // ns
    L7_U64_END_TIME,
    L7_U64_FLOW_ID,
    L7_U64_RRT,             // us (head.rrt)
    L7_U64_SYSCALL_REQ,
    L7_U64_SYSCALL_RESP,
    // OTel ids transcoded to binary at decode (hex strings on the wire):
    // 16-byte trace id as two words, 8-byte span id. Zero = absent or
    // non-hex (then the raw string falls back to the pool columns).
    L7_U64_TRACE_HI,
    L7_U64_TRACE_LO,
    L7_U64_SPAN_ID_B,
    L7_U64_N
};

// ---- u32 columns (int32 fields stored as two's complement) ----
enum {
    L7_U32_VTAP_ID = 0,
    L7_U32_IP4_0,
    L7_U32_IP4_1,
    L7_U32_EPC_0,
    L7_U32_EPC_1,
    L7_U32_PORT_0,
    L7_U32_PORT_1,
    L7_U32_CODE,          // response code (int32)
    L7_U32_REQ_LEN,
    L7_U32_RESP_LEN,
    L7_U32_REQUEST_ID,
    L7_U32_PID_0,
    L7_U32_PID_1,
    L7_U32_GPID_0,
    L7_U32_GPID_1,
    L7_U32_POD_0,         // agent-reported pod ids
    L7_U32_POD_1,
    L7_U32_REQ_TCP_SEQ,
    L7_U32_RESP_TCP_SEQ,
    L7_U32_CAP_REQ_BYTE,
    L7_U32_CAP_RESP_BYTE,
    L7_U32_FLAGS,
    L7_U32_BIZ_TYPE,
    L7_U32_N
};

// ---- u8 columns ----
enum {
    L7_U8_TAP_SIDE = 0,
    L7_U8_TAP_TYPE,
    L7_U8_PROTOCOL,       // l4
    L7_U8_L7_PROTOCOL,    // head.proto
    L7_U8_MSG_TYPE,       // head.msg_type
    L7_U8_STATUS,         // resp.status
    L7_U8_DIR_SCORE,
    L7_U8_IS_IPV6,
    L7_U8_N
};

// ---- string-reference columns (into the batch payload buffer) ----
enum {
    L7_STR_REQ_TYPE = 0,
    L7_STR_DOMAIN,
    L7_STR_RESOURCE,
    L7_STR_ENDPOINT,
    L7_STR_EXCEPTION,
    L7_STR_RESULT,
    L7_STR_VERSION,
    L7_STR_TRACE_ID,
    L7_STR_SPAN_ID,
    L7_STR_PARENT_SPAN_ID,
    L7_STR_XREQ_0,
    L7_STR_XREQ_1,
    L7_STR_UA,            // http_user_agent
    L7_STR_REFERER,
    L7_STR_SERVICE_NAME,
    L7_STR_PKNAME_0,
    L7_STR_PKNAME_1,
    L7_STR_BIZ_CODE,
    L7_STR_IP6_0,         // 16-byte v6 address, pooled (empty for v4 rows)
    L7_STR_IP6_1,
    L7_STR_N
};

#define L7_MAX_ATTRS 16

// string-dict domains (the SmartEncoding per-field namespaces)
enum {
    DICT_DOM_REQ_TYPE = 0,
    DICT_DOM_DOMAIN,
    DICT_DOM_RESOURCE,
    DICT_DOM_ENDPOINT,
    DICT_DOM_VERSION,
    DICT_DOM_SERVICE_NAME,
    DICT_DOM_ATTR_NAME,
    DICT_DOM_ATTR_VALUE,
    DICT_DOM_EXCEPTION,
    DICT_DOM_PKNAME,
    DICT_DOM_N
};

// dict-encoded u32 ID columns written by the intern kernel (K3)
enum {
    L7_DID_REQ_TYPE = 0,
    L7_DID_DOMAIN,
    L7_DID_RESOURCE,
    L7_DID_ENDPOINT,
    L7_DID_VERSION,
    L7_DID_SERVICE_NAME,
    L7_DID_N
};

// KnowledgeGraph columns (K2 join output), per side (0=client,1=server):
enum {
    KG_POD_ID = 0,
    KG_POD_NODE_ID,
    KG_POD_NS_ID,
    KG_POD_GROUP_ID,
    KG_POD_CLUSTER_ID,
    KG_DEVICE_TYPE,
    KG_DEVICE_ID,
    KG_SUBNET_ID,
    KG_HOST_ID,
    KG_AZ_ID,
    KG_SERVICE_ID,
    KG_GPROCESS_ID,
    KG_VALS_N
};

// pool positions of the trace-id fallback columns (the index of
// trace_id/span_id within the pooled subset of the string columns —
// python twin l7_schema.POOL_POS, sync-tested)
#define L7_POOL_TRACE_ID 2
#define L7_POOL_SPAN_ID 3
#define L7_POOL_PARENT_SPAN_ID 4
#define L7_POOL_X_REQUEST_ID_0 5
#define L7_POOL_X_REQUEST_ID_1 6

// L7_U8_STATUS values that count as errors (python twin:
// wire/const_enums.py)
#define STATUS_SERVER_ERROR 3u
#define STATUS_CLIENT_ERROR 4u

#define DICT_ID_INVALID 0xFFFFFFFFu
// String refs carry 16 bits of length: a string keeps at most 65535 bytes.
// Rule for the pooled columns (K4, k_pool_gather):
//  - str_lens[c, row] is declared int16 but holds the length's UNSIGNED
//    16-bit pattern, so 32768..65535 read negative through the declared
//    type. Every reader reinterprets it as u16 (dfseg.h seg_pool_str,
//    query/engine.py, executor.py, tracemap.py). Nothing is clamped to
//    32767: the column is lossless up to the ref's own limit.
//  - str_rowref[row] packs (pool offset, min(row total, 65535)). Only the
//    offset is load-bearing: a row's extent is the sum of its str_lens, and
//    a row whose pooled total exceeds 65535 still stores every byte.
// Python twin of this rule: store/l7_schema.py, ops/ref.py pool_gather_ref.
#define STR_REF_PACK(off, len) \
    ((((uint64_t)(off)) << 16) | ((len) > 0xFFFFu ? 0xFFFFu : (uint64_t)(len)))
#define STR_REF_OFF(r) ((uint64_t)(r) >> 16)
#define STR_REF_LEN(r) ((uint32_t)((r) & 0xFFFFu))
