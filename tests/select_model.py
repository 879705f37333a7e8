"""graph_select in plain Python: the reference's selector parser (src/graph_selector_parse.c) and evaluator
(src/graph_selector_eval.c) restated — a tokenizer with the same look-ahead, queue traversals with the same depth maps.
The checker of tests/test_select.py and bench_select.py; tests/test_select_model.py holds it to the rows and error strings
the compiled reference gave (tests/golden/select.json.gz).  Works on bytes: the reference reads C strings.

A program is the postfix form mn_select_parse returns: a list of (op, name or None, depth_up, depth_down), atoms in
source order."""
from collections import deque

NODE, ANCESTORS, DESCENDANTS, BOTH, CLOSURE, UNION, INTERSECT, COMPLEMENT = range(8)
DIRECTIONS = ("self", "ancestor", "descendant", "both", "closure", "selected", "selected", "selected")
INT_MAX = 2**31 - 1

_LETTERS = frozenset(b"abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ")
_DIGITS = frozenset(b"0123456789")
_START = _LETTERS | _DIGITS | frozenset(b"_")
_INSIDE = _START | frozenset(b".-")


class SelectError(ValueError):
    pass


class _Lexer:
    def __init__(self, text):
        self.s = text + b"\0"
        self.pos = 0
        self.kind, self.start, self.len = "eof", 0, 0

    def _blanks(self):
        while self.s[self.pos] in b" \t":
            self.pos += 1

    def next(self):
        self._blanks()
        c = self.s[self.pos]
        self.start = self.pos
        if c == 0:
            self.kind, self.len = "eof", 0
        elif c in b"+@,":
            self.kind, self.len = chr(c), 1
            self.pos += 1
        elif c in _START:
            while self.s[self.pos] in _INSIDE:
                self.pos += 1
            self.len = self.pos - self.start
            self.kind = "name"
            if self.s[self.start:self.pos] == b"not":
                self._blanks()  # the look-ahead moves the position for good
                if self.s[self.pos] not in b"\0,)":
                    self.kind = "not"
        else:
            raise SelectError(b"graph_select: unexpected character '" + bytes([c]) + b"' at position %d" % self.pos)

    def text(self):
        return self.s[self.start:self.start + self.len]

    def is_int(self):
        return self.kind == "name" and self.len > 0 and all(c in _DIGITS for c in self.text())

    def save(self):
        return self.pos, self.kind, self.start, self.len

    def restore(self, saved):
        self.pos, self.kind, self.start, self.len = saved


def _atom(lx, out):
    at = pre = suf = False
    up = down = -1
    if lx.kind == "@":
        at = True
        lx.next()
    if lx.kind == "+":
        pre = True
        lx.next()
    elif lx.is_int():
        value, saved = min(int(lx.text()), INT_MAX), lx.save()
        lx.next()
        if lx.kind == "+":
            up, pre = value, True
            lx.next()
        else:
            lx.restore(saved)
    if lx.kind != "name":
        raise SelectError(b"graph_select: expected node name at position %d" % lx.start)
    name = lx.text()
    lx.next()
    if lx.kind == "+":
        saved = lx.save()
        lx.next()
        if lx.is_int():
            suf, down = True, min(int(lx.text()), INT_MAX)
            lx.next()
        elif lx.kind in ("eof", ","):
            suf = True
        else:
            lx.restore(saved)  # the plus opens the next term
    if at:
        out.append((CLOSURE, name, -1, -1))
    elif pre and suf:
        out.append((BOTH, name, up, down))
    elif pre:
        out.append((ANCESTORS, name, up, -1))
    elif suf:
        out.append((DESCENDANTS, name, -1, down))
    else:
        out.append((NODE, name, -1, -1))


def _term(lx, out):
    if lx.kind == "not":
        lx.next()
        _atom(lx, out)
        out.append((COMPLEMENT, None, -1, -1))
        return
    _atom(lx, out)
    while lx.kind == ",":
        lx.next()
        _atom(lx, out)
        out.append((INTERSECT, None, -1, -1))


def parse(text):
    """selector text (bytes or str) → program; SelectError carries the reference's message as bytes in args[0]"""
    if isinstance(text, str):
        text = text.encode("utf-8", "surrogateescape")
    text = text.split(b"\0", 1)[0]
    if not text:
        raise SelectError(b"graph_select: empty selector expression")
    lx, out = _Lexer(text), []
    lx.next()
    _term(lx, out)
    while lx.kind in ("name", "+", "@", "not"):
        _term(lx, out)
        out.append((UNION, None, -1, -1))
    if lx.kind != "eof":
        raise SelectError(b"graph_select: unexpected token at position %d" % lx.start)
    return out


# ───────────────────────── evaluator ─────────────────────────

def _walk(lists, seeds, limit, result, depths):
    """bfs_forward / bfs_backward (:153-228): a queue from the seeds in index order into `result`, which may hold nodes
    already; depths None = no depth map, and then every depth reads as 0"""
    q = deque()
    for i in sorted(seeds):
        result.add(i)
        q.append(i)
        if depths is not None:
            depths[i] = 0
    while q:
        cur = q.popleft()
        d = depths[cur] if depths is not None else 0
        if limit >= 0 and d >= limit:
            continue
        for v in lists[cur]:
            if v not in result:
                result.add(v)
                if depths is not None:
                    depths[v] = d + 1
                q.append(v)


def _tree(prog):
    stack = []
    for op, name, up, down in prog:
        if op <= CLOSURE:
            stack.append((op, name, up, down))
        elif op == COMPLEMENT:
            stack.append((op, stack.pop()))
        else:
            right = stack.pop()
            stack.append((op, stack.pop(), right))
    assert len(stack) == 1
    return stack[0]


def _eval(t, n, out, inn, find, depths):
    """eval_ast (:278-481): → the set; depths (a list of -1, or None) is the caller's depth map"""
    op = t[0]
    result = set()
    if op <= CLOSURE:
        _, name, up, down = t
        x = find(name)
        if x < 0:
            raise SelectError((b"graph_select: node '" + name + b"' not found")[:255])
        if op == NODE:
            result.add(x)
            if depths is not None:
                depths[x] = 0
        elif op == ANCESTORS:
            _walk(inn, {x}, up, result, depths)
        elif op == DESCENDANTS:
            _walk(out, {x}, down, result, depths)
        elif op == BOTH:
            d_up, d_down = [-1] * n, [-1] * n
            _walk(inn, {x}, up, result, d_up)
            _walk(out, {x}, down, result, d_down)
            if depths is not None:
                for i in range(n):
                    both = [d for d in (d_up[i], d_down[i]) if d >= 0]
                    if both:
                        depths[i] = min(both)
        else:
            desc = set()
            _walk(out, {x}, -1, desc, None)
            _walk(inn, desc, -1, result, depths)
            result |= desc
            if depths is not None:
                depths[x] = 0
        return result
    if op == COMPLEMENT:
        return set(range(n)) - _eval(t[1], n, out, inn, find, None)
    left = _eval(t[1], n, out, inn, find, None)
    right = _eval(t[2], n, out, inn, find, None)
    return left | right if op == UNION else left & right


def evaluate(prog, n, out, inn, find):
    """selector_eval (:511-543): → ([(node, depth)] in ascending node index, direction); find(name bytes) → index or -1"""
    direction = DIRECTIONS[prog[-1][0]]
    if n == 0:
        return [], direction
    depths = [-1] * n
    got = _eval(_tree(prog), n, out, inn, find, depths)
    return [(i, depths[i] if depths[i] >= 0 else 0) for i in sorted(got)], direction


def lists_of(n, src, dst):
    out, inn = [[] for _ in range(n)], [[] for _ in range(n)]
    for s, d in zip(src, dst):
        out[int(s)].append(int(d))
        inn[int(d)].append(int(s))
    return out, inn


def select_indices(n, src, dst, expr, names=None):
    """what Graph.select gives: (node list, depth list, direction) — or SelectError; names None = decimal indices"""
    out, inn = lists_of(n, src, dst)
    if names is None:
        def find(name):
            return int(name) if name.isdigit() and name == b"%d" % int(name) and int(name) < n else -1
    elif callable(names):
        def find(name):
            i = int(names(name))
            return i if 0 <= i < n else -1
    else:
        index = {}
        for i, nm in enumerate(names):
            index.setdefault(nm.encode() if isinstance(nm, str) else nm, i)

        def find(name):
            return index.get(name, -1)
    rows, direction = evaluate(parse(expr), n, out, inn, find)
    return [r[0] for r in rows], [r[1] for r in rows], direction


def text_select(table_rows, expr):
    """graph_select over an edge table's (src, dst) rows → [[node, depth, direction]]: ids are the values' text in first-seen
    order, a row's src before its dst; rows with a NULL endpoint are skipped (graph_data_load, direction 'both')"""
    ids, index, src, dst = [], {}, [], []
    for s, d in table_rows:
        if s is None or d is None:
            continue
        for v in (s, d):
            k = str(v).encode()
            if k not in index:
                index[k] = len(ids)
                ids.append(str(v))
        src.append(index[str(s).encode()])
        dst.append(index[str(d).encode()])
    prog = parse(expr)
    out, inn = lists_of(len(ids), src, dst)
    rows, direction = evaluate(prog, len(ids), out, inn, lambda name: index.get(name, -1))
    return [[ids[i], d, direction] for i, d in rows]
