"""Shared by tests/test_program_fuzz_cpu.py and tests/test_gpu_program_fuzz.py: seeded random SDF programs.  An SDF program is
data the caller hands over, so the interpreter's input space is the set of VALID programs (include/sdfgrid.h, "SDF programs");
this module draws from it, restates the header's validity rule, edits programs into neighbours that may be invalid, and counts
what a set of programs reaches.  numpy only: nothing of the library is called and no device is needed.

* `corpus(seed, n)`: n valid programs [(opcode, operands)] in tests/program_ref.py's form, each with a box.  A program is grown
  as a postfix sequence by a state machine over (values on the stack, open frames and their kinds, instructions left): at every
  step any instruction is allowed that keeps the program completable in the instructions left, so every shape the header allows
  can occur -- combinators that consume values pushed outside the open frame, MATERIAL anywhere, frames around nothing.  It is
  not emitted from a tree.  Lengths cycle through LENGTHS (1 and SDFV_PROGRAM_MAX_OPS both occur).
* `extreme_corpus(seed, n)`: the same shapes (the same structure stream), operands from the legal edges -- "operands are finite"
  is all the header asks: subnormal and tiny k and radii, radius 0 and negative, a zero plane normal, a singular matrix, s near
  1e-19 and 1e19, operands at +-3e38.
* `first_error(ops, bb)`: the header's rule for sdfv_program_create, restated.
* `mutations(rng, ops)`: one-instruction edits of a valid program.
* `depth_table(programs)`, `crossing_combinators(ops)`: what a set of programs reaches.
* `describe(ops, bb)`: the program as Program builder calls, for failure messages.

An instruction is (opcode, operands) or, in a mutation, (opcode, operands, (r0, r1, r2)) with its reserved words."""
import os

import numpy as np

import program_ref as R

F = np.float32
PRIMITIVES = (R.SPHERE, R.CUBE, R.BOX, R.CYLINDER, R.TORUS, R.PLANE)
COMBINATORS = (R.UNION, R.INTERSECT, R.SUBTRACT, R.SMOOTH_UNION, R.SMOOTH_SUBTRACT)
ON_TOP = (R.ROUND, R.SHELL, R.POP_SCALE)              # one value in, one value out
PUSHES, POPS = (R.PUSH_AFFINE, R.PUSH_SCALE), (R.POP, R.POP_SCALE)
NAMES = {R.SPHERE: "sphere", R.CUBE: "cube", R.BOX: "box", R.CYLINDER: "cylinder", R.TORUS: "torus", R.PLANE: "plane",
         R.PUSH_AFFINE: "push_affine", R.PUSH_SCALE: "push_scale", R.POP: "pop", R.POP_SCALE: "pop_scale", R.UNION: "union",
         R.INTERSECT: "intersect", R.SUBTRACT: "subtract", R.SMOOTH_UNION: "smooth_union", R.SMOOTH_SUBTRACT: "smooth_subtract",
         R.ROUND: "round", R.SHELL: "shell", R.MATERIAL: "material"}
N_OPERANDS = {R.SPHERE: 1, R.CUBE: 1, R.BOX: 3, R.CYLINDER: 2, R.TORUS: 2, R.PLANE: 4, R.PUSH_AFFINE: 12, R.PUSH_SCALE: 2, R.POP: 0,
              R.POP_SCALE: 1, R.UNION: 0, R.INTERSECT: 0, R.SUBTRACT: 0, R.SMOOTH_UNION: 1, R.SMOOTH_SUBTRACT: 1, R.ROUND: 1,
              R.SHELL: 1, R.MATERIAL: 6}
POPS_VALUES = {op: 2 for op in COMBINATORS}
POPS_VALUES.update({op: 1 for op in ON_TOP})
PUSHES_VALUES = {op: 1 for op in PRIMITIVES + COMBINATORS + ON_TOP}

LENGTHS = (1, 2, 3, 5, 8, 13, 21, 34, 55, 89, 144, 233, 256)
assert LENGTHS[-1] == R.MAX_OPS
# Consecutive programs 2i and 2i + 1 share a box (the grid-pass test passes one over a grid loaded with the other).
BOXES = ((-1.0, -1.0, -1.0, 1.0, 1.0, 1.0), (-1.0, -0.9, -0.8, 1.0, 0.9, 0.8), (-0.75, -1.0, -0.5, 1.25, 1.0, 1.0))

DEFAULT_SEED = 20261019
OTHER_SEEDS = (1, 2, 3)                               # the CPU test holds the coverage conditions for these too
# The smallest number of whole cycles of LENGTHS at which DEFAULT_SEED and OTHER_SEEDS all meet the conditions of
# tests/test_program_fuzz_cpu.py::test_the_corpus_is_what_it_claims (found by running that test's check at 1, 2, ... cycles).
CORPUS_CYCLES = 3
CORPUS_SIZE = CORPUS_CYCLES * len(LENGTHS)


def seed():
    """The corpus seed: a constant, or SDFV_SOAK_SEED (tools/soak.sh varies it)."""
    return int(os.environ.get("SDFV_SOAK_SEED", DEFAULT_SEED))


def size():
    """Programs per corpus: CORPUS_SIZE, or SDFV_SOAK_TRIALS rounded up to whole cycles of LENGTHS."""
    trials = os.environ.get("SDFV_SOAK_TRIALS")
    return CORPUS_SIZE if trials is None else -(-max(int(trials), 1) // len(LENGTHS)) * len(LENGTHS)


def f32(v):
    return float(F(v))


# ---- operands ----
class Ordinary:
    """Operands a modeller would write, rounded to f32."""

    def __init__(self, rng):
        self.rng = rng

    def u(self, lo, hi):
        return f32(self.rng.uniform(lo, hi))

    def size(self):                                   # radii and half extents: about [0.05, 0.9], the larger ones more often
        return f32(0.05 + 0.85 * self.rng.beta(2.0, 1.5))

    def primitive(self, op):
        if op in (R.SPHERE, R.CUBE):
            return (self.size(),)
        if op == R.BOX:
            return (self.size(), self.size(), self.size())
        if op == R.CYLINDER:
            return (self.size(), self.size())
        if op == R.TORUS:
            return (self.u(0.2, 0.9), self.u(0.05, 0.4))
        n = self.rng.normal(size=3)
        n /= np.linalg.norm(n)
        return (f32(n[0]), f32(n[1]), f32(n[2]), self.u(-0.5, 0.5))

    def affine(self):
        """The inverse of a rigid placement, built in float64 and then rounded: q' = R^T (q - t)."""
        t = self.rng.uniform(-0.45, 0.45, 3)
        if self.rng.random() < 0.25:
            rot = np.eye(3)
        else:
            q, _ = np.linalg.qr(self.rng.normal(size=(3, 3)))
            rot = q * np.sign(np.linalg.det(q))
        rt = rot.T
        m = np.concatenate([rt, -(rt @ t)[:, None]], axis=1)
        return tuple(f32(v) for v in m.reshape(-1))

    def scale(self):
        s = F(self.rng.uniform(0.5, 1.6))
        return float(s), float(F(1.0) / s)            # inv_s as Program.push_scale computes it

    def k(self):
        return self.u(0.01, 0.3)

    def on_top(self, op):
        return (self.u(0.01, 0.15),) if op == R.ROUND else (self.u(0.03, 0.2),)

    def material(self):
        return tuple(self.u(-0.3, 1.5) for _ in range(6))   # partly out of [0, 1]: the packing clamps


SUB, TINY, BIG = 1e-41, 3e-38, 3e38                  # subnormal; normal with a subnormal quarter; the largest the tests use
assert 0 < F(SUB) < np.finfo(F).tiny and F(TINY) >= np.finfo(F).tiny > F(TINY) * F(0.25) > 0


class Extreme(Ordinary):
    """Operands from the legal edges, each with probability `p`, ordinary ones otherwise."""

    def __init__(self, rng, p):
        super().__init__(rng)
        self.p = p

    def edge(self, choices):
        return f32(choices[self.rng.integers(len(choices))]) if self.rng.random() < self.p else None

    def size(self):
        e = self.edge((SUB, TINY, 0.0, -0.25, -SUB, BIG, -BIG))
        return super().size() if e is None else e

    def primitive(self, op):
        a = super().primitive(op)
        if op == R.PLANE and self.rng.random() < self.p:
            pick = self.rng.integers(4)
            if pick == 0:
                return (0.0, 0.0, 0.0, a[3])          # a zero normal
            if pick == 1:
                return (f32(SUB), f32(-SUB), 0.0, f32(SUB))
            if pick == 2:
                return a[:3] + (f32(BIG * (1 if self.rng.random() < 0.5 else -1)),)
            return (f32(BIG), 0.0, 0.0, a[3])
        if op == R.TORUS and self.rng.random() < self.p:
            return (self.size(), self.size())
        return a

    def affine(self):
        m = list(super().affine())
        if self.rng.random() < self.p:
            pick = self.rng.integers(4)
            if pick == 0:
                m[0:3] = m[4:7]                        # two equal rows: singular
            elif pick == 1:
                m = [0.0] * 12                         # everything maps to the origin
            elif pick == 2:
                m[3 + 4 * int(self.rng.integers(3))] = f32(BIG * (1 if self.rng.random() < 0.5 else -1))
            else:
                m[int(self.rng.integers(12))] = f32(SUB)
        return tuple(m)

    def scale(self):
        if self.rng.random() < self.p:
            s = F((1e-19, 1e19, 3e-19, 2.5e18)[self.rng.integers(4)])
            inv = F(1.0) / s
            assert np.isfinite(inv) and inv > 0 and s > 0
            return float(s), float(inv)
        return super().scale()

    def k(self):
        e = self.edge((SUB, TINY, 1.4e-45, BIG))
        return super().k() if e is None else e

    def on_top(self, op):
        e = self.edge((SUB, 0.0, -0.125, BIG, -BIG, TINY))
        return super().on_top(op) if e is None else (e,)

    def material(self):
        m = list(super().material())
        if self.rng.random() < self.p:
            m[int(self.rng.integers(6))] = f32((BIG, -BIG, SUB, -0.0)[self.rng.integers(4)])
        return tuple(m)


# ---- the state machine ----
def _to_finish(values, frames):
    """The fewest instructions that end a program from here: close every frame, leave one value."""
    return frames + (1 if values == 0 else values - 1)


def _structure(rng, length):
    """`length` opcodes of a valid program, with for every frame-closing opcode the index of the push it closes.  At each step the
    candidates are all opcodes the header allows whose successor state can still be finished in the instructions left; the
    weights steer the value depth towards a target that moves between 1 and the maximum, so that every opcode meets every
    depth."""
    ops, closes, twins = [], {}, {}
    values, frames = 0, []                             # frames: (index of the push, its opcode)
    target = int(rng.integers(1, R.MAX_VALUES + 1))
    forced = []
    for pc in range(length):
        left = length - pc - 1                         # instructions after this one
        cand = {}
        if forced:                                     # the rest of a tie (below)
            op = forced.pop(0)
            ops.append(op)
            values += PUSHES_VALUES.get(op, 0) - POPS_VALUES.get(op, 0)
            continue

        def allow(op, weight, v, f):
            if 0 <= v <= R.MAX_VALUES and 0 <= f <= R.MAX_FRAMES and _to_finish(v, f) <= left:
                cand[op] = weight

        nf = len(frames)
        climb = values < target
        for op in PRIMITIVES:
            allow(op, 3.0 if climb else 0.4, values + 1, nf)
        if values >= 2:
            for op in COMBINATORS:
                allow(op, 0.3 if climb else 2.5, values - 1, nf)
        if values >= 1:
            allow(R.ROUND, 0.7, values, nf)
            allow(R.SHELL, 0.35, values, nf)
        for op in PUSHES:
            allow(op, 0.9, values, nf + 1)
        if frames:
            if frames[-1][1] == R.PUSH_AFFINE:
                allow(R.POP, 1.3, values, nf - 1)
            elif values >= 1:
                allow(R.POP_SCALE, 1.6, values, nf - 1)
        allow(R.MATERIAL, 1.0, values, nf)
        if not cand:                                   # a PUSH_SCALE frame over an empty stack with nothing left but its close
            raise AssertionError((length, pc, values, frames))
        keys = sorted(cand)
        w = np.array([cand[k] for k in keys])
        op = keys[int(rng.choice(len(keys), p=w / w.sum()))]
        ops.append(op)
        values += PUSHES_VALUES.get(op, 0) - POPS_VALUES.get(op, 0)
        # A tie: now and then a primitive is followed by MATERIAL, the same primitive once more (_fill gives it the same
        # operands) and a combinator, so that the combinator sees a.d == b.d bit for bit at EVERY point under two different
        # materials and the header's tie rule alone picks one.  Random operands never tie.
        if op in PRIMITIVES and left >= 3 and values + 1 <= R.MAX_VALUES and _to_finish(values, len(frames)) <= left - 3 and rng.random() < 0.12:
            forced = [R.MATERIAL, op, COMBINATORS[int(rng.integers(len(COMBINATORS)))]]
            twins[pc + 2] = pc
        if op in PUSHES:
            frames.append((pc, op))
        elif op in POPS:
            closes[pc] = frames.pop()[0]
        if values == target or rng.random() < 0.05:
            target = int(rng.integers(1, R.MAX_VALUES + 1))
    assert values == 1 and not frames and not forced
    return ops, closes, twins


def _fill(rng, ops, closes, twins, draw):
    out = []
    for pc, op in enumerate(ops):
        if op in PRIMITIVES:
            a = out[twins[pc]][1] if pc in twins else draw.primitive(op)
        elif op == R.PUSH_AFFINE:
            a = draw.affine()
        elif op == R.PUSH_SCALE:
            a = draw.scale()
        elif op == R.POP_SCALE:
            a = (out[closes[pc]][1][0],)               # the s of the frame it closes
        elif op in (R.SMOOTH_UNION, R.SMOOTH_SUBTRACT):
            a = (draw.k(),)
        elif op in (R.ROUND, R.SHELL):
            a = draw.on_top(op)
        elif op == R.MATERIAL:
            a = draw.material()
        else:
            a = ()
        out.append((op, tuple(float(v) for v in a)))
    return out


def corpus(seed_value, n):
    """-> [(ops, bb)]: n valid programs with ordinary operands."""
    out = []
    for i in range(n):
        rng = np.random.default_rng([int(seed_value), i])
        ops, closes, twins = _structure(rng, LENGTHS[i % len(LENGTHS)])
        out.append((_fill(rng, ops, closes, twins, Ordinary(rng)), BOXES[(i // 2) % len(BOXES)]))
    return out


def extreme_corpus(seed_value, n, ordinary_points=None):
    """-> [(ops, bb)]: the shapes of corpus(seed_value, n) with operands from the legal edges.  The header's promise for the
    ORDINARY points of a batch (tests/program_ref.py, assert_records_under_the_nan_rule) presupposes that they stay numbers, so
    the operands of a program are redrawn, with fewer edges each time, until program_ref.run gives no NaN and no undecided
    material on `ordinary_points` (default: the ordinary points of program_ref.odd_batch)."""
    if ordinary_points is None:
        pts, mask = R.odd_batch()
        ordinary_points = pts[mask]
    out = []
    for i in range(n):
        rng = np.random.default_rng([int(seed_value), i])
        ops, closes, twins = _structure(rng, LENGTHS[i % len(LENGTHS)])
        for attempt in range(12):
            draw_rng = np.random.default_rng([int(seed_value), i, attempt])
            prog = _fill(draw_rng, ops, closes, twins, Extreme(draw_rng, 0.5 * 0.6 ** attempt))
            rec, decided = R.run(prog, ordinary_points, want_decided=True)
            if decided.all() and not np.isnan(rec[:, 0]).any():
                break
        else:
            raise AssertionError(("no numeric draw", seed_value, i))
        out.append((prog, BOXES[(i // 2) % len(BOXES)]))
    return out


def has_edge_operands(ops):
    """Whether some operand of the program is subnormal, zero where a size is expected, negative where one is, or huge."""
    for op, a in ops:
        if op in (R.MATERIAL, R.POP, R.UNION, R.INTERSECT, R.SUBTRACT):
            continue
        v = np.abs(np.array(a, F))
        if ((v > 0) & (v < 1e-18)).any() or (v > 1e18).any():
            return True
        if op in (R.SPHERE, R.CUBE, R.ROUND, R.SHELL) and a[0] <= 0:
            return True
    return False


# ---- the header's validity rule ----
def first_error(ops, bb, n=None):
    """None for a program sdfv_program_create accepts, else (index, kind): the first offending instruction and why, with index
    None for the rules about the whole program ("count": n == 0 or n > SDFV_PROGRAM_MAX_OPS; "box"; "open frames" and "values"
    at the end).  The header lists what is refused, not in which order two faults of ONE instruction are reported; the order
    here is opcode, reserved words, operands finite, the operand's sign, the frame stack, the frame's kind, the value stack."""
    n = len(ops) if n is None else n
    if n == 0 or n > R.MAX_OPS:
        return None, "count"
    b = np.array(bb, F)
    if len(b) != 6 or not np.isfinite(b).all() or not (b[3:] > b[:3]).all():
        return None, "box"
    values, frames = 0, []
    for i, ins in enumerate(ops[:n]):
        op, a = ins[0], np.zeros(12, F)
        with np.errstate(over="ignore"):
            a[:len(ins[1])] = np.array(ins[1], np.float64).astype(F)
        if not (R.SPHERE <= op <= R.MATERIAL):
            return i, "unknown opcode"
        if len(ins) > 2 and any(ins[2]):
            return i, "reserved"
        if not np.isfinite(a).all():
            return i, "not finite"
        if op in (R.SMOOTH_UNION, R.SMOOTH_SUBTRACT) and not a[0] > 0:
            return i, "k <= 0"
        if op == R.PUSH_SCALE and not (a[0] > 0 and a[1] > 0):
            return i, "s <= 0"
        if op == R.POP_SCALE and not a[0] > 0:
            return i, "s <= 0"
        if op in PUSHES:
            if len(frames) == R.MAX_FRAMES:
                return i, "frame overflow"
            frames.append(op)
        elif op in POPS:
            if not frames:
                return i, "frame underflow"
            if (frames[-1] == R.PUSH_SCALE) != (op == R.POP_SCALE):
                return i, "POP closes a PUSH_SCALE" if op == R.POP else "POP_SCALE closes a PUSH_AFFINE"
            frames.pop()
        if values < POPS_VALUES.get(op, 0):
            return i, "value underflow"
        values += PUSHES_VALUES.get(op, 0) - POPS_VALUES.get(op, 0)
        if values > R.MAX_VALUES:
            return i, "value overflow"
    if frames:
        return None, "open frames"
    if values != 1:
        return None, "values"
    return None


ERROR_KINDS = ("unknown opcode", "reserved", "not finite", "k <= 0", "s <= 0", "value underflow", "value overflow", "frame underflow",
               "frame overflow", "POP closes a PUSH_SCALE", "POP_SCALE closes a PUSH_AFFINE", "count", "open frames", "values", "box")


# ---- neighbours of a valid program ----
def mutations(rng, ops, n=20):
    """-> n of [(what, ops)]: `ops` with one instruction deleted, duplicated, swapped with its neighbour, given another opcode,
    one operand set to NaN, inf, 0 or a negative value, or a reserved word set.  Some stay valid, some do not."""
    out = []
    kinds = ("delete", "duplicate", "swap", "swap", "opcode", "operand", "operand", "reserved")
    for _ in range(n):
        prog = [tuple(ins) for ins in ops]
        i = int(rng.integers(len(prog)))
        kind = kinds[int(rng.integers(len(kinds)))]
        if kind == "delete":
            del prog[i]
        elif kind == "duplicate":
            prog.insert(i, prog[i])
        elif kind == "swap":
            j = min(i + 1, len(prog) - 1)
            prog[i], prog[j] = prog[j], prog[i]
        elif kind == "opcode":
            new = int(rng.choice([0, 19, 0xffffffff])) if rng.random() < 0.15 else int(rng.integers(R.SPHERE, R.MATERIAL + 1))
            a = prog[i][1]
            if rng.random() < 0.5:                     # with operands that suit the new opcode, or with the old ones
                a = tuple(f32(v) for v in rng.uniform(0.1, 0.9, N_OPERANDS.get(new, 0)))
            prog[i] = (new, a)
        elif kind == "operand":
            # among the operands the opcode reads, or any of the twelve (an unused one must still be finite)
            k = int(rng.integers(max(N_OPERANDS[prog[i][0]], 1))) if rng.random() < 0.7 else int(rng.integers(12))
            a = list(prog[i][1]) + [0.0] * (12 - len(prog[i][1]))
            a[k] = (float("nan"), float("inf"), float("-inf"), 0.0, -0.0, -0.5, f32(-SUB))[int(rng.integers(7))]
            prog[i] = (prog[i][0], tuple(a))
            kind = f"operand {k} = {a[k]}"
        else:
            r = [0, 0, 0]
            r[int(rng.integers(3))] = int(rng.choice([1, 0x80000000, 0xffffffff]))
            prog[i] = (prog[i][0], prog[i][1], tuple(r))
        out.append((f"{kind} at {i}", prog))
    return out


# ---- what a set of programs reaches ----
def depth_table(programs):
    """-> (values, frames): {(opcode, value depth before it): count} for the opcodes that push or take values, and
    {(opcode, frame depth before it): count} for the frame opcodes."""
    values_t, frames_t = {}, {}
    for ops in programs:
        v = f = 0
        for ins in ops:
            op = ins[0]
            if op in PUSHES_VALUES:
                values_t[op, v] = values_t.get((op, v), 0) + 1
            if op in PUSHES + POPS:
                frames_t[op, f] = frames_t.get((op, f), 0) + 1
            v += PUSHES_VALUES.get(op, 0) - POPS_VALUES.get(op, 0)
            f += (op in PUSHES) - (op in POPS)
    return values_t, frames_t


def required_cells():
    """The cells a corpus must reach: primitive x depth 0..7, combinator x 2..8, ROUND / SHELL / POP_SCALE x 1..8; PUSH_* x frame
    depth 0..3, POP* x 1..4."""
    values = [(op, d) for op in PRIMITIVES for d in range(0, R.MAX_VALUES)]
    values += [(op, d) for op in COMBINATORS for d in range(2, R.MAX_VALUES + 1)]
    values += [(op, d) for op in ON_TOP for d in range(1, R.MAX_VALUES + 1)]
    frames = [(op, d) for op in PUSHES for d in range(0, R.MAX_FRAMES)] + [(op, d) for op in POPS for d in range(1, R.MAX_FRAMES + 1)]
    return values, frames


def format_tables(values_t, frames_t):
    lines = ["opcode           value depth before it: " + " ".join(f"{d:5d}" for d in range(R.MAX_VALUES + 1))]
    for op in PRIMITIVES + COMBINATORS + ON_TOP:
        lines.append(f"{NAMES[op]:40s}" + " ".join(f"{values_t.get((op, d), 0):5d}" for d in range(R.MAX_VALUES + 1)))
    lines.append("opcode           frame depth before it: " + " ".join(f"{d:5d}" for d in range(R.MAX_FRAMES + 1)))
    for op in PUSHES + POPS:
        lines.append(f"{NAMES[op]:40s}" + " ".join(f"{frames_t.get((op, d), 0):5d}" for d in range(R.MAX_FRAMES + 1)))
    return "\n".join(lines)


def crossing_combinators(ops):
    """Indices of the combinators that consume a value pushed BEFORE the innermost frame open at the time."""
    out, values, frames = [], [], []                   # values: index of the instruction that made each; frames: index of the push
    for pc, (op, *_) in enumerate(ops):
        if op in PUSHES:
            frames.append(pc)
        elif op in POPS:
            frames.pop()
        if op in COMBINATORS:
            b, a = values.pop(), values.pop()
            if frames and min(a, b) < frames[-1]:
                out.append(pc)
            values.append(pc)
        elif op in ON_TOP:
            values[-1] = pc
        elif op in PRIMITIVES:
            values.append(pc)
    return out


def ties(ops):
    """{combinator opcode: count} of the exact ties of the program: a primitive, MATERIAL, the same primitive with the same
    operands, the combinator."""
    out = {}
    for pc in range(3, len(ops)):
        if (ops[pc][0] in COMBINATORS and ops[pc - 2][0] == R.MATERIAL and ops[pc - 3][0] in PRIMITIVES
                and tuple(ops[pc - 3][:2]) == tuple(ops[pc - 1][:2])):
            out[ops[pc][0]] = out.get(ops[pc][0], 0) + 1
    return out


def materials_inside_frames(ops):
    """Indices of the MATERIAL instructions between a push and its pop."""
    out, f = [], 0
    for pc, (op, *_) in enumerate(ops):
        f += (op in PUSHES) - (op in POPS)
        if op == R.MATERIAL and f:
            out.append(pc)
    return out


# ---- what the comparisons run on ----
def builder(PM, ops, bb):
    """A Program builder (sdf-viewer_amd.program) holding `ops` as they are."""
    b = PM.Program(bb)
    b.ops = [(int(op), tuple(float(v) for v in a)) for op, a in ops]
    return b


def moderate(points):
    """The points whose coordinates are 0 or of ordinary magnitude.  Every point of program_ref.points() is finite; its blocks of
    tiny and huge coordinates are there to overflow and underflow (inf - inf is a NaN under any rotation), so "no NaN anywhere"
    is a property a corpus can have on the rest only."""
    mag = np.abs(points)
    return ((mag == 0) | ((mag > 1e-15) & (mag < 1e3))).all(axis=1)


def changes_sign(ops, bb, n=13):
    """Whether the program's distance takes both signs on the n^3 lattice over its box."""
    d = R.run(ops, R.grid_positions((n, n, n), bb[:3], bb[3:]), True)[:, 0]
    return bool((d < 0).any() and (d > 0).any())


def share(programs, count=13, stride=3):
    """A route's share of a corpus when the whole would take too long: at least `count` programs that change sign on their
    lattice, every stride-th first -- with the default sizes that is one program of every length."""
    picked = [i for i in range(0, len(programs), stride) if changes_sign(*programs[i])]
    rest = [i for i in range(len(programs)) if i not in picked and changes_sign(*programs[i])]
    return sorted((picked + rest)[:max(count, len(picked))])


MARCH_SIZE = (43, 27)                                  # neither a multiple of 8: the right and bottom tiles hold lanes off the image


def march_cameras(pkg, bb, width=MARCH_SIZE[0], height=MARCH_SIZE[1]):
    """(an orbit camera that sees the whole box with sky around it, a close one whose frame the box overfills)."""
    c = [(bb[a] + bb[a + 3]) / 2.0 for a in range(3)]
    aspect = width / height
    orbit = pkg.camera_look_at(eye=(c[0] + 1.125, c[1] + 1.35, c[2] + 2.25), target=c, aspect=aspect)
    close = pkg.camera_look_at(eye=(c[0] - 0.9, c[1] + 0.5, c[2] + 1.4), target=c, aspect=aspect, fovy_degrees=60.0)
    return orbit, close


def render_params(pkg, bb):
    return pkg.default_render_params(pkg.make_grid((256, 256, 256), bb[:3], bb[3:]))


# ---- failure messages ----
def describe(ops, bb=None):
    """The program as Program builder calls, one per line (floats print as the shortest text that reads back to the same f32
    value's double, so the text rebuilds the program bit for bit)."""
    lines = ["Program()" if bb is None else f"Program({tuple(float(v) for v in bb)!r})"]
    for ins in ops:
        op, a = ins[0], tuple(float(v) for v in ins[1])
        name = NAMES.get(op)
        text = ", ".join(repr(v) for v in a)
        plain = name is not None and len(a) == N_OPERANDS[op] and len(ins) == 2
        if plain and op == R.PUSH_AFFINE:
            lines.append(f".push_affine(({text}))")
        elif plain and op == R.PUSH_SCALE and float(F(1.0) / F(a[0])) == a[1]:
            lines.append(f".push_scale({a[0]!r})")
        elif plain and op != R.PUSH_SCALE:
            lines.append(f".{name}({text})")
        else:
            lines.append(f".op({op}{', ' if a else ''}{text})" + (f"  # reserved words {ins[2]}" if len(ins) > 2 else ""))
    return "\n".join(lines)


def label(seed_value, index, ops, bb=None, kind="corpus"):
    """What every failure message of the fuzz tests carries: enough to rebuild the program from the log."""
    return f"{kind}(seed={seed_value})[{index}], {len(ops)} instructions:\n{describe(ops, bb)}\n"
