"""SmartEncoding tag dictionary (string interning).

GPU side: one open-addressing table (u64 hash keys; DICT ID == slot index)
shared by all dict domains, written by the intern kernel (K3). New entries
are emitted to a side buffer as (domain<<56|slot, packed batch str-ref); the
host harvests them after each batch into the authoritative id<->string maps
used for query-time hydration and string-literal -> id filter compilation.

This realizes the reference's SmartEncoding write path: integer IDs stored in
columns (grpc_platformdata.go / flow_tag_writer.go roles), with query-time
re-hydration replacing ClickHouse dictGet (tag/translation.go:101).
"""
from __future__ import annotations

from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

from . import l7_schema as S

EMIT_CAP = 1 << 20


def str_hash_py(data: bytes, seed: int) -> int:
    """Python twin of dfgpu.hip str_hash (used by the CPU reference ops)."""
    M = (1 << 64) - 1
    h = (seed ^ 0x27D4EB2F165667C5 ^ (len(data) * 0x9E3779B97F4A7C15)) & M
    i = 0
    n = len(data)
    while i + 8 <= n:
        k = int.from_bytes(data[i:i + 8], "little")
        h ^= (k * 0xC2B2AE3D27D4EB4F) & M
        h = ((h << 31) | (h >> 33)) & M
        h = (h * 0x9E3779B185EBCA87) & M
        i += 8
    tail = 0
    for j in range(n - i):
        tail |= data[i + j] << (8 * j)
    h ^= (tail * 0x165667B19E3779F9) & M
    h ^= h >> 33
    h = (h * 0xFF51AFD7ED558CCD) & M
    h ^= h >> 29
    h = (h * 0xC4CEB9FE1A85EC53) & M
    h ^= h >> 32
    return h if h else 1


def domain_seed(domain: int) -> int:
    return (0x9E3779B97F4A7C15 * (domain + 1)) & ((1 << 64) - 1)


class DictArena:
    """One dictionary domain's strings on a device, for k_dict_match (K16:
    LIKE / REGEXP on dictionary tags): the entries' bytes back to back and
    three columns per entry, byte offset (u32), id (u32) and length (u16).

    Built lazily and only at query time: TagDictionary.arena() hands new
    entries over as (id, bytes) in `pending`, upload() appends them with one
    host-to-device copy of the bytes and one of the columns. Buffers grow by
    doubling; old contents are copied on the device."""

    MAX_BYTES = (1 << 32) - 1           # offsets are u32

    def __init__(self, device):
        self.device = torch.device(device)
        self.n = 0                      # entries uploaded
        self.nbytes = 0                 # arena bytes in use
        self.data = torch.zeros(0, dtype=torch.uint8, device=self.device)
        self.off = torch.zeros(0, dtype=torch.int32, device=self.device)
        self.ids = torch.zeros(0, dtype=torch.int32, device=self.device)
        self.lens = torch.zeros(0, dtype=torch.int16, device=self.device)
        self.pending: List[Tuple[int, bytes]] = []
        # counters (tests and benchmarks read them)
        self.h2d_copies = 0
        self.h2d_bytes = 0
        self.uploads = 0

    @staticmethod
    def _grown(t: torch.Tensor, used: int, need: int, floor: int):
        if need <= t.numel():
            return t
        cap = max(t.numel(), floor)
        while cap < need:
            cap *= 2
        new = torch.zeros(cap, dtype=t.dtype, device=t.device)
        new[:used].copy_(t[:used])      # device to device
        return new

    def upload(self) -> int:
        """Append the pending entries. -> how many."""
        new = self.pending
        if not new:
            return 0
        self.pending = []
        k = len(new)
        lens = np.fromiter((len(s) for _, s in new), dtype=np.int64, count=k)
        if int(lens.max()) > 0xFFFF:
            raise RuntimeError("dictionary entry longer than 65535 bytes")
        total = int(lens.sum())
        if self.nbytes + total > self.MAX_BYTES:
            raise RuntimeError("dictionary arena exceeds 4 GiB")
        offs = self.nbytes + np.cumsum(lens) - lens
        cols = np.empty(10 * k, dtype=np.uint8)
        cols[:4 * k].view(np.uint32)[:] = offs
        cols[4 * k:8 * k].view(np.uint32)[:] = np.fromiter(
            (i for i, _ in new), dtype=np.int64, count=k)
        cols[8 * k:].view(np.uint16)[:] = lens
        self.data = self._grown(self.data, self.nbytes, self.nbytes + total,
                                1 << 12)
        self.off = self._grown(self.off, self.n, self.n + k, 1 << 8)
        self.ids = self._grown(self.ids, self.n, self.n + k, 1 << 8)
        self.lens = self._grown(self.lens, self.n, self.n + k, 1 << 8)
        if total:
            joined = np.frombuffer(b"".join(s for _, s in new),
                                   dtype=np.uint8)
            self.data[self.nbytes:self.nbytes + total].copy_(
                torch.from_numpy(joined.copy()))
            self.h2d_copies += 1
            self.h2d_bytes += total
        dcols = torch.from_numpy(cols).to(self.device)
        self.h2d_copies += 1
        self.h2d_bytes += cols.nbytes
        n = self.n
        self.off[n:n + k].copy_(dcols[:4 * k].view(torch.int32))
        self.ids[n:n + k].copy_(dcols[4 * k:8 * k].view(torch.int32))
        self.lens[n:n + k].copy_(dcols[8 * k:].view(torch.int16))
        self.n += k
        self.nbytes += total
        self.uploads += 1
        return k


class TagDictionary:
    """Per-shard tag dictionary: GPU table + host id<->string maps."""

    def __init__(self, capacity_pow2: int = 1 << 22, device: str = "cpu"):
        assert capacity_pow2 & (capacity_pow2 - 1) == 0
        self.capacity = capacity_pow2
        self.device = device
        dev = torch.device(device)
        self.tkeys = torch.zeros(capacity_pow2, dtype=torch.int64, device=dev)
        self.emit = torch.zeros((EMIT_CAP, 2), dtype=torch.int64, device=dev)
        self.emit_ctr = torch.zeros(1, dtype=torch.int32, device=dev)
        # host maps: (domain, id) -> string ; (domain, string) -> id
        self.id_to_str: Dict[Tuple[int, int], bytes] = {}
        self.str_to_id: Dict[Tuple[int, bytes], int] = {}
        # overflow count (table-full events observed at harvest)
        self.dropped = 0
        # entries discovered since the last cross-shard sync
        self.pending_sync: List[Tuple[int, int, bytes]] = []
        # K16 device arenas, {domain: {device: DictArena}}, and how many
        # entries of id_to_str (in insertion order) they have been offered
        self._arenas: Dict[int, Dict[str, DictArena]] = {}
        self._arena_seen = 0

    def n_entries(self) -> int:
        return len(self.id_to_str)

    def arena(self, domain: int, device) -> DictArena:
        """The domain's strings on `device`, caught up with id_to_str.

        Nothing on the ingest path knows about arenas: whatever put entries
        into id_to_str (harvest, import_entries, a restored checkpoint), a
        dict keeps insertion order and entries are never removed, so the
        entries past `_arena_seen` are exactly the new ones. They are read
        from the dict's end, so a catch-up costs O(new entries), and O(1)
        when there are none."""
        n = len(self.id_to_str)
        new = n - self._arena_seen
        if new:
            if self._arenas:
                import itertools
                tail = list(itertools.islice(
                    reversed(self.id_to_str.items()), new))
                for (dom, slot), s in reversed(tail):
                    for a in self._arenas.get(dom, {}).values():
                        a.pending.append((slot, s))
            self._arena_seen = n
        per_dev = self._arenas.setdefault(domain, {})
        a = per_dev.get(str(device))
        if a is None:
            # first use: the one walk over the whole dictionary
            a = per_dev[str(device)] = DictArena(device)
            a.pending = [(slot, s) for (dom, slot), s
                         in self.id_to_str.items() if dom == domain]
        a.upload()
        return a

    def harvest(self, payload) -> int:
        """Drain the emit buffer after a batch. `payload` is the batch's
        raw bytes — host numpy, or a DEVICE uint8 tensor (routed batches
        have no host copy: only the emitted slices transfer, a few bytes
        per NEW dictionary entry instead of a full-batch D2H)."""
        cnt = int(self.emit_ctr[0].item())
        if cnt == 0:
            return 0
        take = min(cnt, EMIT_CAP)
        rows = self.emit[:take].cpu().numpy()
        import torch
        is_dev = isinstance(payload, torch.Tensor) and \
            payload.device.type != "cpu"
        for tag, ref in rows:
            tag = int(tag) & 0xFFFFFFFFFFFFFFFF
            ref = int(ref) & 0xFFFFFFFFFFFFFFFF
            dom = tag >> 56
            slot = tag & 0xFFFFFFFF
            off, ln = ref >> 16, ref & 0xFFFF
            if is_dev:
                sbytes = bytes(payload[off:off + ln].cpu().numpy())
            else:
                sbytes = payload[off:off + ln].tobytes()
            self.id_to_str[(dom, slot)] = sbytes
            self.str_to_id[(dom, sbytes)] = slot
            self.pending_sync.append((dom, slot, sbytes))
        if cnt > EMIT_CAP:
            self.dropped += cnt - EMIT_CAP
        self.emit_ctr.zero_()
        return take

    def lookup_id(self, domain: int, value: bytes) -> Optional[int]:
        return self.str_to_id.get((domain, value))

    def lookup_str(self, domain: int, ident: int) -> Optional[bytes]:
        if ident == S.DICT_ID_INVALID or ident < 0:
            return None
        return self.id_to_str.get((domain, ident))

    def hydrate(self, domain: int, ids) -> List[Optional[str]]:
        out = []
        for i in ids:
            i = int(i)
            if i < 0 or i == S.DICT_ID_INVALID:
                out.append(None)
            else:
                b = self.id_to_str.get((domain, i & 0xFFFFFFFF))
                out.append(b.decode("utf-8", "replace") if b is not None else None)
        return out

    # ---- cross-shard sync (parallel/dict_sync.py drives this) ----
    def export_entries(self, since: int = 0) -> List[Tuple[int, int, bytes]]:
        """All (domain, id, string) entries; `since` reserved for deltas."""
        return [(d, i, s) for (d, i), s in self.id_to_str.items()]

    def import_entries(self, entries) -> None:
        """Merge remote (domain, id, string) entries for query-side
        hydration of remote shards (ids are shard-local; callers keep these
        in per-shard maps)."""
        for d, i, s in entries:
            self.id_to_str.setdefault((d, i), s)
            self.str_to_id.setdefault((d, s), i)
