"""AirBuilder: assembles a constraint program (include/ronk_ntt.h "constraint programs") from expressions.

    b = AirBuilder()
    a, nxt = b.base(0), b.base(0, rot=1)
    b.constrain(nxt - a * a * b.x - b.imm(3), EXCEPT_LAST)
    b.constrain(a - b.chal(0), FIRST)
    ops, imm, n_regs, n_constraints = b.assemble()

Leaves are base(c, rot), ext(c, rot), periodic(p, rot), chal(k), imm(v) and x; expressions support + - * and unary -, with Python integers taken as
immediates.  Equal subexpressions are one node (a + b and b + a, a * b and b * a are equal) and are computed once; registers are
allocated greedily in evaluation order and freed at the last use of a value.  A program that needs more than 16 live values
raises AirError.  Pure Python: nothing here touches the device."""

MOV, ADD, SUB, MUL, NEG, EMIT = range(6)
REG, BASE, EXT, CHAL, IMM, X, PER = range(7)
ALL, FIRST, LAST, EXCEPT_LAST = range(4)
MAX_REGS, MAX_IMM, MAX_OPS, MAX_CONSTRAINTS = 16, 256, 4096, 64


class AirError(ValueError):
    pass


def operand(kind, index=0, rot=0):
    if not (0 <= index < 256 and -2048 <= rot < 2048):
        raise AirError("operand index %d or rot %d does not fit the op word" % (index, rot))
    return kind | index << 4 | (rot & 0xFFF) << 12


class Expr:
    """a node of a builder: a leaf (`leaf` its operand word) or an operation on earlier nodes"""
    __slots__ = ("builder", "code", "args", "leaf")

    def __init__(self, builder, code, args, leaf):
        self.builder, self.code, self.args, self.leaf = builder, code, args, leaf

    def _bin(self, code, other, swap=False):
        other = self.builder._lift(other)
        return self.builder._node(code, (other, self) if swap else (self, other))

    def __add__(self, o): return self._bin(ADD, o)
    def __radd__(self, o): return self._bin(ADD, o, True)
    def __sub__(self, o): return self._bin(SUB, o)
    def __rsub__(self, o): return self._bin(SUB, o, True)
    def __mul__(self, o): return self._bin(MUL, o)
    def __rmul__(self, o): return self._bin(MUL, o, True)
    def __neg__(self): return self.builder._node(NEG, (self,))


class AirBuilder:
    def __init__(self):
        self._nodes, self._imm, self._constraints = {}, [], []
        self.x = self._leaf(operand(X))

    # ---- leaves
    def _leaf(self, word):
        key = ("leaf", word)
        if key not in self._nodes:
            self._nodes[key] = Expr(self, None, (), word)
        return self._nodes[key]

    def base(self, c, rot=0):
        return self._leaf(operand(BASE, c, rot))

    def ext(self, c, rot=0):
        return self._leaf(operand(EXT, c, rot))

    def periodic(self, p, rot=0):
        """periodic column p of the handle (ronk_air_create_per): a base element"""
        return self._leaf(operand(PER, p, rot))

    def chal(self, k):
        return self._leaf(operand(CHAL, k))

    def imm(self, v):
        v = int(v)
        if v not in self._imm:
            if len(self._imm) == MAX_IMM:
                raise AirError("more than %d distinct immediates" % MAX_IMM)
            self._imm.append(v)
        return self._leaf(operand(IMM, self._imm.index(v)))

    def _lift(self, v):
        if isinstance(v, Expr):
            if v.builder is not self:
                raise AirError("an expression of another builder")
            return v
        return self.imm(v)

    def _node(self, code, args):
        ids = tuple(id(a) for a in args)
        key = (code,) + (tuple(sorted(ids)) if code in (ADD, MUL) else ids)
        if key not in self._nodes:
            self._nodes[key] = Expr(self, code, args, None)
        return self._nodes[key]

    # ---- constraints
    def constrain(self, expr, kind=ALL):
        if kind not in (ALL, FIRST, LAST, EXCEPT_LAST):
            raise AirError("a constraint kind is ALL, FIRST, LAST or EXCEPT_LAST")
        if len(self._constraints) == MAX_CONSTRAINTS:
            raise AirError("more than %d constraints" % MAX_CONSTRAINTS)
        self._constraints.append((self._lift(expr), kind))
        return len(self._constraints) - 1

    def assemble(self):
        """-> (ops, imm, n_regs, n_constraints)"""
        if not self._constraints:
            raise AirError("a program has at least one constraint")
        # how often every computed node is read: once per reading op, each node being computed once
        uses, seen, stack = {}, set(), [e for e, _ in self._constraints]
        for e, _ in self._constraints:
            uses[id(e)] = uses.get(id(e), 0) + 1
        while stack:
            e = stack.pop()
            if id(e) in seen or e.leaf is not None:
                continue
            seen.add(id(e))
            for a in e.args:
                uses[id(a)] = uses.get(id(a), 0) + 1
                stack.append(a)
        ops, reg_of, free, high = [], {}, list(range(MAX_REGS - 1, -1, -1)), [0]

        def read(e):
            """the operand word of a value that is ready; its register is freed with its last read"""
            if e.leaf is not None:
                return e.leaf
            r = reg_of[id(e)]
            uses[id(e)] -= 1
            if uses[id(e)] == 0:
                free.append(r)
                free.sort(reverse=True)
            return operand(REG, r)

        def compute(root):
            # iterative post-order: a node is computed when all its arguments are ready
            todo = [(root, False)]
            while todo:
                e, ready = todo.pop()
                if e.leaf is not None or id(e) in reg_of:
                    continue
                if not ready:
                    todo.append((e, True))
                    todo.extend((a, False) for a in reversed(e.args))
                    continue
                words = [read(a) for a in e.args]
                if not free:
                    raise AirError("the program needs more than %d live registers" % MAX_REGS)
                r = free.pop()
                high[0] = max(high[0], r + 1)
                reg_of[id(e)] = r
                ops.append(e.code | r << 8 | words[0] << 16 | (words[1] << 40 if len(words) > 1 else 0))

        for j, (e, kind) in enumerate(self._constraints):
            compute(e)
            ops.append(EMIT | kind << 8 | read(e) << 16 | j << 40)
        if len(ops) > MAX_OPS:
            raise AirError("the program has %d ops, more than %d" % (len(ops), MAX_OPS))
        return ops, list(self._imm), high[0], len(self._constraints)
