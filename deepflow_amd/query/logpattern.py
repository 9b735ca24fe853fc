"""The template of a log body (K14): one definition for both log stores.

A body is cut into tokens at delimiter bytes; a token that holds an ASCII
digit is a variable and collapses to one WILDCARD symbol, everything else
stands for itself. Two bodies belong to one pattern when their symbol
streams are equal. The host store groups by the stream itself
(template_symbols); the GPU store groups by its 64-bit hash (template_key,
computed by k_log_patterns in ops/csrc/dflog.hip from the pool's bytes).
64-bit key identity is accepted, as it is for every dictionary here: two
streams with one key would be counted as one pattern on the GPU store.

All of it works on bytes: the pool's bytes on the GPU store, and
body.encode("utf-8", "replace") on the host store.

- delimiters: every byte <= 0x20 and the 13 bytes of `"'(),;:=[]{}|`.
  Everything else is not, `.`, `-`, `/`, `_`, `<`, `>` and all bytes
  >= 0x80 included;
- digits: the ASCII bytes 0..9 only;
- only the first PATTERN_PREFIX bytes of a body are looked at: a token cut
  by the cap ends there, digits beyond the cap do not count, and a body
  longer than the cap gets one trailing TRUNC symbol;
- symbol stream: a delimiter byte emits itself, a token with a digit emits
  WILDCARD, any other token emits its bytes;
- key: FNV-1a over the symbols in 64 bits, then mix64 (ops/csrc/dfhash.h),
  0 mapped to 1 (0 is EMPTY_KEY in ops/csrc/dftable.h). It needs one pass
  and O(1) state: remember h at a token's start, fold the token's bytes,
  and at its end replace h by fold(saved, WILDCARD) if it held a digit.
"""
from __future__ import annotations

from typing import Iterable, Tuple

PATTERN_PREFIX = 512            # df_log_pattern_prefix() in dflog.hip
WILDCARD = 0x100
TRUNC = 0x101
MAX_PATTERNS_LIMIT = 1 << 30
DELIMITERS = frozenset(range(0x21)) | frozenset(b"\"'(),;:=[]{}|")

FNV_OFFSET = 0xCBF29CE484222325
FNV_PRIME = 0x100000001B3
_M64 = (1 << 64) - 1
_DIGITS = frozenset(b"0123456789")


def mix64(z: int) -> int:
    """mix64 of ops/csrc/dfhash.h."""
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)


def template_symbols(body: bytes) -> Tuple[int, ...]:
    """The symbol stream of a body: ints 0..255, WILDCARD and TRUNC."""
    body = bytes(body)
    head = body[:PATTERN_PREFIX]
    out = []
    start = 0                   # index in `out` where the open token began
    digit = False
    for c in head:
        if c in DELIMITERS:
            if digit:
                out[start:] = [WILDCARD]
                digit = False
            out.append(c)
            start = len(out)
        else:
            out.append(c)
            if c in _DIGITS:
                digit = True
    if digit:
        out[start:] = [WILDCARD]
    if len(body) > PATTERN_PREFIX:
        out.append(TRUNC)
    return tuple(out)


def symbols_key(symbols: Iterable[int]) -> int:
    h = FNV_OFFSET
    for s in symbols:
        h = ((h ^ s) * FNV_PRIME) & _M64
    return mix64(h) or 1


def template_key(body: bytes) -> int:
    """The 64-bit key k_log_patterns gives the body; never 0."""
    return symbols_key(template_symbols(body))


def render(symbols: Iterable[int]) -> str:
    """Literal runs decoded as UTF-8 (errors replaced), WILDCARD as `<*>`,
    TRUNC as `<...>`. Not injective: a body may hold a literal `<*>`."""
    parts = []
    run = bytearray()
    for s in symbols:
        if s < 0x100:
            run.append(s)
            continue
        if run:
            parts.append(run.decode("utf-8", "replace"))
            run = bytearray()
        parts.append("<*>" if s == WILDCARD else "<...>")
    if run:
        parts.append(run.decode("utf-8", "replace"))
    return "".join(parts)


def check_max_patterns(max_patterns) -> int:
    """patterns()'s max_patterns: a power of two in 1..2^30 (the slots of
    the GPU store's query-scoped table, 32 bytes each; the host store only
    validates it)."""
    if isinstance(max_patterns, bool) or not isinstance(max_patterns, int) \
            or not 1 <= max_patterns <= MAX_PATTERNS_LIMIT \
            or max_patterns & (max_patterns - 1):
        raise ValueError("max_patterns must be a power of two in 1..2^30")
    return max_patterns
