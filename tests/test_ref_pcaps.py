"""Replay the reference's golden pcap fixtures through the C++ agent engine.
This validates our parsers against real captures from the reference's own
test corpus (agent/resources/test/flow_generator); the captures the tests
use are stored under tests/golden/flow_generator."""
import os
import struct

from deepflow_amd.agent import Agent
from deepflow_amd.wire import pb, flow_log, framing

FIX = os.path.join(os.path.dirname(os.path.abspath(__file__)),
                   "golden", "flow_generator")


def read_pcap(path):
    """Minimal pcap reader -> [(ts_ns, frame)] supporting us/ns magic,
    both endiannesses, and linktype ethernet/linux-sll(113)."""
    data = open(path, "rb").read()
    magic = struct.unpack("<I", data[:4])[0]
    if magic == 0xA1B2C3D4:
        endian, scale = "<", 1000
    elif magic == 0xA1B23C4D:
        endian, scale = "<", 1
    elif magic == 0xD4C3B2A1:
        endian, scale = ">", 1000
    else:
        raise ValueError("bad pcap magic")
    linktype = struct.unpack(endian + "I", data[20:24])[0]
    pos = 24
    out = []
    while pos + 16 <= len(data):
        ts_s, ts_frac, incl, orig = struct.unpack(endian + "IIII",
                                                  data[pos:pos + 16])
        pos += 16
        frame = data[pos:pos + incl]
        pos += incl
        if linktype == 113:  # LINUX_SLL -> fake ethernet
            # sll: 2 pkttype, 2 arphrd, 2 addrlen, 8 addr, 2 proto
            proto = frame[14:16]
            frame = b"\x02\xbb\x00\x00\x00\x01\x02\xaa\x00\x00\x00\x01" + \
                proto + frame[16:]
        out.append((ts_s * 10**9 + ts_frac * scale, frame))
    return out


def replay(path):
    a = Agent(vtap_id=1)
    for ts, frame in read_pcap(path):
        a.packet(frame, ts)
    a.tick(1 << 62)
    l7 = [pb.decode(r, flow_log.APP_PROTO_LOGS_DATA)
          for r in framing.iter_records(a.drain(1))]
    l4 = [pb.decode(r, flow_log.TAGGED_FLOW)
          for r in framing.iter_records(a.drain(0))]
    stats = a.stats()
    a.close()
    return l7, l4, stats


def test_dns_pcap():
    l7, l4, stats = replay(f"{FIX}/dns/a-and-ns.pcap")
    assert stats["parse_errors"] == 0
    assert len(l7) >= 1
    assert all(r["base"]["head"]["proto"] == 120 for r in l7)
    domains = {r["req"]["domain"] for r in l7}
    assert any("." in d for d in domains), domains


def test_http_pcap():
    l7, l4, stats = replay(f"{FIX}/http/client-ip.pcap")
    assert len(l7) == 1
    r = l7[0]
    assert r["base"]["head"]["proto"] == 20
    assert r["req"]["req_type"] == "POST"
    assert r["req"]["resource"].startswith("/biz-inquiry-bff/")
    assert r["resp"]["code"] == 200


def test_redis_pcap():
    l7, l4, stats = replay(f"{FIX}/redis/redis.pcap")
    assert len(l7) >= 1
    assert all(r["base"]["head"]["proto"] == 80 for r in l7)
    cmds = {r["req"]["req_type"] for r in l7}
    assert cmds, cmds


def test_mysql_pcap():
    path = f"{FIX}/mysql"
    caps = sorted(f for f in os.listdir(path) if f.endswith(".pcap"))
    hits = 0
    for c in caps[:6]:
        l7, _, _ = replay(f"{path}/{c}")
        hits += sum(1 for r in l7 if r["base"]["head"]["proto"] == 60)
    assert hits >= 1


def test_l4_flow_metrics_from_pcap():
    l7, l4, stats = replay(f"{FIX}/redis/redis.pcap")
    assert len(l4) >= 1
    f = l4[0]["flow"]
    assert f["metrics_peer_src"]["packet_count"] > 0
    assert f["flow_key"]["port_dst"] == 6379 or \
        f["flow_key"]["port_src"] == 6379


def test_grpc_pcaps():
    """HTTP/2 + HPACK + gRPC against the reference's own golden captures
    (expected values from the matching .result files)."""
    l7, _, _ = replay(f"{FIX}/http/grpc-unary.pcap")
    assert len(l7) == 1
    r = l7[0]
    assert r["base"]["head"]["proto"] == 41  # gRPC
    assert r["req"]["req_type"] == "POST"
    assert r["req"]["resource"] == "/agent.Synchronizer/Sync"
    assert r["ext_info"]["service_name"] == "agent.Synchronizer"
    assert r["resp"]["code"] == 200

    l7b, _, _ = replay(f"{FIX}/http/grpc-server-stream.pcap")
    assert any(x["req"]["resource"] ==
               "/timeseriesquery.TimeSeriesQueryService/ServerStreamQuery"
               for x in l7b)


def test_grpc_in_agent_session():
    """Synthetic HTTP/2 exchange through the normal packet path."""
    import struct
    from deepflow_amd.agent import Agent
    from deepflow_amd.agent.packets import (eth_ipv4_tcp, SYN, SYNACK,
                                            PSH_ACK)

    def hb(s):  # literal-without-indexing header (name+value raw strings)
        n, v = s
        return bytes([0x00, len(n)]) + n.encode() + \
            bytes([len(v)]) + v.encode()

    req_block = (b"\x83"  # :method POST (indexed 3)
                 + hb((":path", "/svc.Api/Do"))
                 + hb((":authority", "api.local"))
                 + hb(("content-type", "application/grpc")))
    req_frame = struct.pack(">I", len(req_block))[1:] + \
        bytes([1, 0x04]) + struct.pack(">I", 1) + req_block
    resp_block = b"\x88" + hb(("content-type", "application/grpc"))
    resp_frame = struct.pack(">I", len(resp_block))[1:] + \
        bytes([1, 0x04]) + struct.pack(">I", 1) + resp_block
    a = Agent(vtap_id=5)
    t0 = 10**9
    pkts = [
        (eth_ipv4_tcp(0x0A000001, 0x0A000002, 43000, 50051, SYN, 1), t0),
        (eth_ipv4_tcp(0x0A000002, 0x0A000001, 50051, 43000, SYNACK, 2, 2),
         t0 + 10**6),
        (eth_ipv4_tcp(0x0A000001, 0x0A000002, 43000, 50051, PSH_ACK, 2, 3,
                      req_frame), t0 + 2 * 10**6),
        (eth_ipv4_tcp(0x0A000002, 0x0A000001, 50051, 43000, PSH_ACK, 3,
                      2 + len(req_frame), resp_frame), t0 + 6 * 10**6),
    ]
    for frame, ts in pkts:
        a.packet(frame, ts)
    a.tick(10**9 * 100)
    from deepflow_amd.wire import pb, flow_log, framing
    recs = [pb.decode(r, flow_log.APP_PROTO_LOGS_DATA)
            for r in framing.iter_records(a.drain(1))]
    assert len(recs) == 1
    assert recs[0]["base"]["head"]["proto"] == 41
    assert recs[0]["req"]["resource"] == "/svc.Api/Do"
    assert recs[0]["req"]["domain"] == "api.local"
    assert recs[0]["ext_info"]["service_name"] == "svc.Api"
    a.close()


def test_mqtt_pcaps():
    l7, _, _ = replay(f"{FIX}/mqtt/mqtt_pub.pcap")
    types = [r["req"]["req_type"] for r in l7]
    assert "CONNECT" in types and "PUBLISH" in types
    pub = next(r for r in l7 if r["req"]["req_type"] == "PUBLISH")
    assert pub["req"]["resource"] == "bench"
    assert pub["base"]["head"]["proto"] == 101


def test_amqp_pcaps():
    l7, _, _ = replay(f"{FIX}/amqp/amqp1.pcap")
    types = [r["req"]["req_type"] for r in l7]
    assert "ProtocolHeader" in types
    assert any(t.startswith("Connection.") for t in types)
    assert all(r["base"]["head"]["proto"] == 102 for r in l7)


def test_kafka_pcap():
    l7, _, _ = replay(f"{FIX}/kafka/00-produce-v2.pcap")
    assert len(l7) == 1
    assert l7[0]["base"]["head"]["proto"] == 100
    assert l7[0]["req"]["req_type"] == "Produce"


def test_mongo_pcap():
    l7, _, _ = replay(f"{FIX}/mongo/mongo.pcap")
    assert len(l7) >= 10
    assert all(r["base"]["head"]["proto"] == 81 for r in l7)


def test_pgsql_pcaps():
    l7, _, _ = replay(f"{FIX}/postgre/simple_query.pcap")
    assert l7[0]["req"]["resource"].strip().startswith("delete")
    l7e, _, _ = replay(f"{FIX}/postgre/error.pcap")
    assert l7e[0]["resp"]["status"] == 3


def test_memcached_pcap():
    l7, _, _ = replay(f"{FIX}/memcached/memcached.pcap")
    assert [(r["req"]["req_type"], r["req"]["resource"]) for r in l7] == \
        [("set", "foo"), ("get", "foo")]


def test_dubbo_pcap():
    l7, _, _ = replay(f"{FIX}/dubbo/dubbo_hessian2.pcap")
    assert len(l7) == 1
    r = l7[0]
    assert r["base"]["head"]["proto"] == 40
    assert r["req"]["resource"] == "my.demo.service.UserService/login"
    assert r["ext_info"]["service_name"] == "my.demo.service.UserService"
    # dubbo status 20 == OK
    assert r["resp"].get("status", 0) == 0


def test_fastcgi_pcap():
    l7, _, _ = replay(f"{FIX}/fastcgi/fastcgi.pcap")
    assert len(l7) == 1
    assert l7[0]["base"]["head"]["proto"] == 44
    assert l7[0]["req"]["req_type"] == "GET"
    assert l7[0]["resp"]["code"] == 200


def test_rpc_mq_pcaps():
    l7, _, _ = replay(f"{FIX}/brpc/brpc-echo.pcap")
    assert all(r["base"]["head"]["proto"] == 45 for r in l7)
    assert l7[0]["req"]["resource"] == "example.EchoService/Echo"
    assert l7[0]["ext_info"]["service_name"] == "example.EchoService"

    l7, _, _ = replay(f"{FIX}/tars/tars-echo.pcap")
    assert any(r["req"]["resource"] == "tars.tarslog.LogObj/tars_ping"
               for r in l7)

    l7, _, _ = replay(f"{FIX}/sofarpc/sofa-old.pcap")
    assert len(l7) == 1 and l7[0]["base"]["head"]["proto"] == 43
    assert l7[0]["req"]["resource"].startswith("com.alipay.sofa.rpc")

    l7, _, _ = replay(f"{FIX}/rocketmq/rocketmq-send-message-v2.pcap")
    assert len(l7) == 2
    assert all(r["req"]["req_type"] == "SendMessageV2" for r in l7)

    l7, _, _ = replay(f"{FIX}/nats/nats-skywalking.pcap")
    assert any(r["req"]["req_type"] in ("PUB", "HPUB") for r in l7)


def test_zmtp_pcaps():
    # REQ/REP NULL-mechanism session: READY handshake + request/response
    l7, _, stats = replay(f"{FIX}/zmtp/zmtp_null.pcap")
    assert all(r["base"]["head"]["proto"] == 106 for r in l7)
    types = [r["req"]["req_type"] for r in l7]
    assert "READY" in types and "Message" in types
    ready = [r for r in l7 if r["req"]["req_type"] == "READY"]
    assert {r["req"]["resource"] for r in ready} == {"REQ", "REP"}
    msg = [r for r in l7 if r["req"]["req_type"] == "Message"]
    assert msg and msg[0]["base"]["head"].get("rrt", 0) > 0

    # SUBSCRIBE command carries the topic
    l7, _, _ = replay(f"{FIX}/zmtp/zmtp_subscribe_one.pcap")
    subs = [r["req"]["resource"] for r in l7
            if r["req"]["req_type"] == "SUBSCRIBE"]
    assert subs == ["sports.general"], \
        [r["req"]["req_type"] for r in l7]

    # ERROR command (incl. the libzmq \x5eRROR merge quirk) -> server error
    l7, _, _ = replay(f"{FIX}/zmtp/zmtp_error.pcap")
    errs = [r for r in l7 if r["req"]["req_type"] == "ERROR"]
    assert errs and all(e["resp"].get("status") == 3 for e in errs)
    assert errs[0]["req"]["resource"] == "400"


def test_someip_pcap():
    l7, _, stats = replay(f"{FIX}/some_ip/some_ip.pcap")
    assert l7, "no SOME/IP records"
    assert all(r["base"]["head"]["proto"] == 47 for r in l7)
    # reference .result: request_resource 41 (service), endpoint 20484
    # (method), matched request/response with return code E_OK
    r = l7[0]
    assert r["req"]["req_type"] == "Request"
    assert r["req"]["resource"] == "41/20484"
    assert r["resp"].get("code", 0) == 0
    assert r["base"]["head"].get("rrt", 0) > 0


def test_pulsar_pcaps():
    # IPv6 capture: also exercises the agent's v6 L3 path
    l7, l4, _ = replay(f"{FIX}/pulsar/pulsar-producer.pcap")
    assert all(r["base"]["head"]["proto"] == 105 for r in l7)
    types = {r["req"]["req_type"] for r in l7}
    assert "CONNECT" in types and "SEND" in types
    prod = [r for r in l7 if r["req"]["req_type"] == "PRODUCER"]
    assert prod and prod[0]["req"]["resource"] == \
        "persistent://public/default/my-topic"
    sends = [r for r in l7 if r["req"]["req_type"] == "SEND"]
    assert len(sends) == 10  # ten send/send_receipt pairs in the fixture
    # rrt values line up with the reference .result for the same pairs
    assert sends[0]["base"]["head"]["rrt"] == 11240
    # the L4 flow carries the IPv6 addresses
    assert l4 and l4[0]["flow"]["flow_key"].get("ip6_src")

    l7, _, _ = replay(f"{FIX}/pulsar/pulsar-consumer.pcap")
    subs = [r for r in l7 if r["req"]["req_type"] == "SUBSCRIBE"]
    assert subs and subs[0]["req"]["resource"] == \
        "persistent://public/default/my-topic"


def test_openwire_pcaps():
    l7, _, _ = replay(f"{FIX}/openwire/openwire_loose_producer.pcap")
    assert all(r["base"]["head"]["proto"] == 103 for r in l7)
    types = [r["req"]["req_type"] for r in l7]
    assert "WIREFORMAT_INFO" in types
    assert "CONNECTION_INFO" in types  # loose command matched by corrId
    conn = [r for r in l7 if r["req"]["req_type"] == "CONNECTION_INFO"]
    assert conn[0]["base"]["head"].get("rrt", 0) > 0

    l7, _, _ = replay(f"{FIX}/openwire/openwire_exception.pcap")
    errs = [r for r in l7 if r["resp"].get("status") == 3]
    assert errs, [r["req"]["req_type"] for r in l7]


def test_grpc_segmented_pcap():
    """HEADERS frame followed by a DATA frame split across TCP segments:
    exercises the per-direction carry-over reassembly + the request-flush
    on flow close (.result expects one request record, no response)."""
    l7, _, _ = replay(f"{FIX}/http/grpc-segmented.pcap")
    assert len(l7) == 1
    assert l7[0]["req"]["resource"] == "/agent.Synchronizer/Push"
    assert l7[0]["ext_info"]["service_name"] == "agent.Synchronizer"

    # pure bulk TCP (iperf) must yield no L7 records
    l7, _, stats = replay(f"{FIX}/tcp-segment.pcap")
    assert l7 == [] and stats["parse_errors"] == 0
