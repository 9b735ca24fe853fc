"""Regex patterns for the application-log store (K13): pattern -> DFA.

compile_log_regex() takes a pattern to an *anchored* DFA over byte classes;
"unanchored" is supplied by whoever walks it, by trying every start
position (k_log_regex in ops/csrc/dflog.hip does, and so does
LogRegex.search_py, the plain-Python twin used to test the compiler without
a GPU). The meaning of a pattern is Python's `re` on bytes:

    re.search(pattern.encode("utf-8"), body.encode("utf-8", "replace"),
              re.IGNORECASE if case_insensitive else 0)

so \\d \\w \\s are ASCII, `.` is any byte but \\n and IGNORECASE folds A-Z
only. Case-insensitivity is baked into the byte sets (every positive set is
closed under ASCII case before it is negated); the walker gets no fold
flag.

Supported: literals and escapes, `.`, classes (ranges, negation, \\d\\w\\s
and their negations), ( ) and (?: ) groups, `|`, * + ? {m} {m,} {m,n} with
an optional lazy `?` (laziness cannot change a boolean answer), ^ or \\A as
the first item and $ or \\Z as the last item of the top-level sequence.
Everything else is refused with a ValueError that names the construct.

The parser is CPython's own (its op tree is walked against a whitelist),
the NFA is Thompson's, the DFA comes from subset construction and stops as
soon as it passes the size the kernel stages in LDS.

State 0 is dead, state 1 is the start. Table layout (LogRegex.table(), the
bytes the kernel stages): class_of u8[256], then next u16[n_states *
n_classes] where bit 15 of an entry says that the state it leads to
accepts and the low 15 bits are that state (0: dead).
"""
from __future__ import annotations

import functools
import re
from typing import List, Optional, Tuple

import numpy as np

try:                                    # Python >= 3.11
    import re._parser as _sre_parse
    import re._constants as _sre
except ImportError:                     # pragma: no cover - older Pythons
    import sre_parse as _sre_parse
    import sre_constants as _sre

# the kernel's limits; tests hold them against df_log_re_limits()
MAX_TABLE_BYTES = 32 * 1024             # n_states * n_classes * 2
MAX_PATTERN_BYTES = 256
MAX_CLASSES = 64
_MAX_NFA_STATES = 1 << 14               # a{9999}: refuse before expanding
_CACHE_ENTRIES = 64

DEAD, START = 0, 1
ACCEPT_BIT = 1 << 15
STATE_MASK = ACCEPT_BIT - 1

FLAG_ANCHOR_START = 1
FLAG_ANCHOR_END = 2
FLAG_END_BEFORE_NL = 4                  # `$`: also just before a final \n
FLAG_NULLABLE = 8

_ALL = (1 << 256) - 1
_NL = 1 << 10


def _set_of(pattern: bytes) -> int:
    """The bytes a one-byte pattern matches, as a 256-bit mask: `re` itself
    says what \\d, \\w and \\s are on bytes."""
    rx = re.compile(pattern)
    return sum(1 << b for b in range(256) if rx.match(bytes([b])))


_CATEGORY = {
    _sre.CATEGORY_DIGIT: _set_of(rb"\d"),
    _sre.CATEGORY_NOT_DIGIT: _set_of(rb"\D"),
    _sre.CATEGORY_SPACE: _set_of(rb"\s"),
    _sre.CATEGORY_NOT_SPACE: _set_of(rb"\S"),
    _sre.CATEGORY_WORD: _set_of(rb"\w"),
    _sre.CATEGORY_NOT_WORD: _set_of(rb"\W"),
}

_UPPER = sum(1 << b for b in range(ord("A"), ord("Z") + 1))
_LOWER = _UPPER << 32

_REFUSED_AT = {
    _sre.AT_BOUNDARY: r"\b", _sre.AT_NON_BOUNDARY: r"\B",
}
_REFUSED_OP = {
    "GROUPREF": "backreference", "GROUPREF_EXISTS": "conditional group",
    "GROUPREF_IGNORE": "backreference", "ASSERT": "look-around",
    "ASSERT_NOT": "look-around", "POSSESSIVE_REPEAT": "possessive repeat",
    "ATOMIC_GROUP": "atomic group",
}


def _unsupported(what: str) -> ValueError:
    return ValueError(f"log regex: unsupported construct: {what}")


def _too_complex(why: str) -> ValueError:
    return ValueError(f"log regex: pattern too complex ({why})")


def _close_case(mask: int) -> int:
    return mask | ((mask & _UPPER) << 32) | ((mask & _LOWER) >> 32)


class _Nfa:
    """Thompson NFA: every state has epsilon edges and at most one byte
    edge (set, target)."""

    def __init__(self, fold: bool):
        self.fold = fold
        self.eps: List[List[int]] = []
        self.edge: List[Optional[Tuple[int, int]]] = []

    def state(self) -> int:
        if len(self.eps) >= _MAX_NFA_STATES:
            raise _too_complex("repeat counts expand to too many states")
        self.eps.append([])
        self.edge.append(None)
        return len(self.eps) - 1

    def positive(self, mask: int) -> int:
        return _close_case(mask) if self.fold else mask

    # every builder returns (entry, exit) of a fragment
    def byte_set(self, mask: int) -> Tuple[int, int]:
        a, b = self.state(), self.state()
        self.edge[a] = (mask, b)
        return a, b

    def empty(self) -> Tuple[int, int]:
        a = self.state()
        return a, a

    def class_mask(self, items) -> int:
        mask, negate = 0, False
        for op, av in items:
            if op is _sre.NEGATE:
                negate = True
            elif op is _sre.LITERAL:
                if av > 255:
                    raise _unsupported("a literal outside the byte range")
                mask |= 1 << av
            elif op is _sre.RANGE:
                lo, hi = av
                if hi > 255:
                    raise _unsupported("a range outside the byte range")
                mask |= ((1 << (hi - lo + 1)) - 1) << lo
            elif op is _sre.CATEGORY and av in _CATEGORY:
                mask |= _CATEGORY[av]
            else:
                raise _unsupported(f"class item {op} {av}")
        mask = self.positive(mask)
        return _ALL & ~mask if negate else mask

    def seq(self, items) -> Tuple[int, int]:
        first, last = self.empty()
        for item in items:
            a, b = self.item(item)
            self.eps[last].append(a)
            last = b
        return first, last

    def item(self, item) -> Tuple[int, int]:
        op, av = item
        if op is _sre.LITERAL:
            if av > 255:
                raise _unsupported("a literal outside the byte range")
            return self.byte_set(self.positive(1 << av))
        if op is _sre.NOT_LITERAL:
            return self.byte_set(_ALL & ~self.positive(1 << av))
        if op is _sre.ANY:
            return self.byte_set(_ALL & ~_NL)
        if op is _sre.IN:
            return self.byte_set(self.class_mask(av))
        if op is _sre.BRANCH:
            a, b = self.state(), self.state()
            for alt in av[1]:
                x, y = self.seq(alt)
                self.eps[a].append(x)
                self.eps[y].append(b)
            return a, b
        if op is _sre.SUBPATTERN:
            _group, add_flags, del_flags, sub = av
            if add_flags or del_flags:
                raise _unsupported("inline flags")
            return self.seq(sub)
        if op is _sre.MAX_REPEAT or op is _sre.MIN_REPEAT:
            return self.repeat(*av)
        if op is _sre.AT:
            if av in _REFUSED_AT:
                raise _unsupported(_REFUSED_AT[av])
            raise _unsupported(
                "an anchor that is not the first (^ \\A) or the last "
                "($ \\Z) item of the whole pattern")
        name = str(op)
        raise _unsupported(_REFUSED_OP.get(name, name))

    def repeat(self, lo: int, hi, sub) -> Tuple[int, int]:
        first, last = self.empty()
        for _ in range(lo):
            a, b = self.seq(sub)
            self.eps[last].append(a)
            last = b
        if hi is _sre.MAXREPEAT or hi == _sre.MAXREPEAT:
            a, b = self.seq(sub)
            end = self.state()
            self.eps[last] += [a, end]
            self.eps[b] += [a, end]
            return first, end
        end = self.state()
        for _ in range(hi - lo):
            a, b = self.seq(sub)
            self.eps[last] += [a, end]
            last = b
        self.eps[last].append(end)
        return first, end


def _byte_classes(masks) -> List[int]:
    """Partition 0..255 into the coarsest classes no set in `masks` splits;
    -> one mask per class, ordered by lowest member."""
    classes = [_ALL]
    for m in masks:
        nxt = []
        for c in classes:
            inside, outside = c & m, c & ~m
            if inside:
                nxt.append(inside)
            if outside:
                nxt.append(outside)
        classes = nxt
        if len(classes) > MAX_CLASSES:
            raise _too_complex(f"more than {MAX_CLASSES} byte classes")
    return sorted(classes, key=lambda c: (c & -c))


def _bits(m: int) -> List[int]:
    out = []
    while m:
        low = m & -m
        out.append(low.bit_length() - 1)
        m ^= low
    return out


class LogRegex:
    """A compiled pattern: the tables k_log_regex walks, plus `host`, the
    `re` object with the same meaning (the host store's matcher and the
    oracle)."""

    def __init__(self, pattern: str, case_insensitive: bool,
                 host: "re.Pattern", class_of: np.ndarray, nxt: np.ndarray,
                 accept: np.ndarray, flags: int):
        self.pattern = pattern
        self.case_insensitive = case_insensitive
        self.host = host
        self.class_of = class_of                # u8[256]
        self.next = nxt                         # u16[n_states * n_classes]
        self.accept = accept                    # bool[n_states]
        self.n_classes = int(class_of.max()) + 1
        self.n_states = int(accept.shape[0])
        self.flags = flags
        self.anchor_start = bool(flags & FLAG_ANCHOR_START)
        self.anchor_end = bool(flags & FLAG_ANCHOR_END)
        self.end_before_newline = bool(flags & FLAG_END_BEFORE_NL)
        self.nullable = bool(flags & FLAG_NULLABLE)
        assert nxt.shape[0] == self.n_states * self.n_classes
        assert int(nxt.max(initial=0)) < self.n_states <= STATE_MASK
        assert nxt.nbytes <= MAX_TABLE_BYTES
        packed = nxt | (accept[nxt].astype(np.uint16) << 15)
        self._table = np.concatenate(
            [class_of.view(np.uint8), packed.view(np.uint8)])
        self._packed = packed.tolist()
        self._class_list = class_of.tolist()

    @property
    def matches_everything(self) -> bool:
        """A nullable pattern that is not anchored at both ends matches
        the empty string somewhere in every body."""
        return self.nullable and not (self.anchor_start and self.anchor_end)

    def table(self) -> np.ndarray:
        """class_of, then next with the accept bits folded in (u8 view)."""
        return self._table

    def search_py(self, body: bytes) -> bool:
        """The kernel's walk in plain Python: same tables, same anchor
        rules. Equals bool(self.host.search(body))."""
        if self.matches_everything:
            return True
        n = len(body)
        if n == 0:
            return self.nullable
        cls, nxt, nc = self._class_list, self._packed, self.n_classes
        for q in ((0,) if self.anchor_start else range(n)):
            state, acc, alive = START, self.nullable, True
            acc_before = False
            if not self.anchor_end:
                # the shortest accept from q decides
                for i in range(q, n):
                    e = nxt[state * nc + cls[body[i]]]
                    if e == 0 or e & ACCEPT_BIT:
                        break
                    state = e
                else:
                    continue
                if e:
                    return True
                continue
            for i in range(q, n):
                if i == n - 1:
                    acc_before = acc
                e = nxt[state * nc + cls[body[i]]]
                if e == 0:
                    alive = False
                    break
                state, acc = e & STATE_MASK, bool(e & ACCEPT_BIT)
            if alive and acc:
                return True
            if self.end_before_newline and acc_before and body[-1] == 10:
                return True
        return False


def _compile(pattern: str, fold: bool) -> LogRegex:
    try:
        pat = pattern.encode("utf-8")
    except UnicodeEncodeError as e:
        raise ValueError(f"log regex: pattern is not valid as bytes: {e}")
    if len(pat) > MAX_PATTERN_BYTES:
        raise _too_complex(f"longer than {MAX_PATTERN_BYTES} bytes")
    try:
        host = re.compile(pat, re.IGNORECASE if fold else 0)
        tree = _sre_parse.parse(pat, 0)
    except (re.error, OverflowError, RecursionError) as e:
        raise ValueError(f"log regex: invalid pattern: {e}")
    if tree.state.flags:
        raise _unsupported("inline flags")
    items = list(tree)
    flags = 0
    if items and items[0][0] is _sre.AT and items[0][1] in (
            _sre.AT_BEGINNING, _sre.AT_BEGINNING_STRING):
        flags |= FLAG_ANCHOR_START
        items = items[1:]
    if items and items[-1][0] is _sre.AT and items[-1][1] in (
            _sre.AT_END, _sre.AT_END_STRING):
        flags |= FLAG_ANCHOR_END
        if items[-1][1] is _sre.AT_END:
            flags |= FLAG_END_BEFORE_NL
        items = items[:-1]

    nfa = _Nfa(fold)
    try:
        entry, final = nfa.seq(items)
    except RecursionError:
        raise _too_complex("nested too deeply")
    n_nfa = len(nfa.eps)

    # epsilon closure of every state, as a bit mask of NFA states
    closure = [0] * n_nfa
    for s in range(n_nfa):
        seen, stack = 1 << s, [s]
        while stack:
            for t in nfa.eps[stack.pop()]:
                if not seen >> t & 1:
                    seen |= 1 << t
                    stack.append(t)
        closure[s] = seen

    classes = _byte_classes(sorted({e[0] for e in nfa.edge if e}))
    n_classes = len(classes)
    class_of = np.zeros(256, dtype=np.uint8)
    for k, cm in enumerate(classes):
        class_of[_bits(cm)] = k
    # per NFA state with a byte edge: the closure it leads to, per class
    step = {}
    for s, e in enumerate(nfa.edge):
        if e:
            step[s] = [closure[e[1]] if cm & e[0] else 0 for cm in classes]
    edged = sum(1 << s for s in step)

    cap = MAX_TABLE_BYTES // (2 * n_classes)
    ids = {0: DEAD, closure[entry]: START}
    members = [[], _bits(closure[entry] & edged)]
    accept = [False, bool(closure[entry] >> final & 1)]
    rows: List[List[int]] = [[DEAD] * n_classes]
    todo = 1
    while todo < len(members):
        row = []
        for k in range(n_classes):
            m = 0
            for s in members[todo]:
                m |= step[s][k]
            t = ids.get(m)
            if t is None:
                t = ids[m] = len(members)
                if t >= cap:
                    raise _too_complex(
                        f"its DFA needs more than {MAX_TABLE_BYTES} bytes")
                members.append(_bits(m & edged))
                accept.append(bool(m >> final & 1))
            row.append(t)
        rows.append(row)
        todo += 1
    if accept[START]:
        flags |= FLAG_NULLABLE
    return LogRegex(pattern, fold, host, class_of,
                    np.array(rows, dtype=np.uint16).reshape(-1),
                    np.array(accept, dtype=bool), flags)


_cached = functools.lru_cache(maxsize=_CACHE_ENTRIES)(_compile)


def compile_log_regex(pattern: str,
                      case_insensitive: bool = False) -> LogRegex:
    """Validate and compile. TypeError for a non-str; ValueError for an
    invalid pattern, an unsupported construct (named in the message) or a
    pattern whose DFA exceeds the kernel's limits."""
    if not isinstance(pattern, str):
        raise TypeError("regex is a str")
    return _cached(pattern, bool(case_insensitive))


def check_log_regex(regex: Optional[str],
                    case_insensitive: bool = False) -> Optional[LogRegex]:
    """The `regex` argument of search()/histogram() -> a compiled pattern,
    or None when it constrains nothing (None or ""). The one validator of
    both stores."""
    if regex is None:
        return None
    if not isinstance(regex, str):
        raise TypeError("regex is a str")
    return compile_log_regex(regex, case_insensitive) if regex else None
