"""
The scalar side of the three order-2 sample loops of the headline k_sweep instantiation (TRANSLATE, order 2, float32,
pitch 121), read off the disassembly of the built library the way csrc/check_isa.py reads it.

A sample loop is an innermost natural loop of the kernel's control-flow graph that holds exactly 36 `ds_read_b64`: four
samples of nine taps.  There are three: the interior loop with the sample mask, the interior loop over all-finite windows
(CLEAN) and the bounded loop.  Per iteration (one chunk of four points) each of them
  * holds no `s_nop` (the wait state the compiler wants after an inline-asm statement is filled with work);
  * spends at most two scalar instructions on the point address (one 64-bit pointer bump: the four prefetches take
    immediate offsets);
  * keeps its vector instruction count: 140 / 127 / 156;
and the two interior loops wait on lgkmcnt(0) exactly four times, once per gather (the prefetch of the next point is
drained by that wait and has none of its own).
"""
import importlib.util
import os
import re

import pytest

HEADLINE = "k_sweepILi0ELi2EfLb0ELb0ELi121EE"
LLVM = os.environ.get("ROCM_LLVM_BIN", "/opt/rocm/lib/llvm/bin")
_BRANCH = re.compile(r"s_(c?branch\w*)\s+(\d+)")


def _check_isa():
    from euispice_coreg_amd import _lib
    spec = importlib.util.spec_from_file_location("check_isa", os.path.join(os.path.dirname(_lib.LIB_PATH), "csrc",
                                                                          "check_isa.py"))
    chk = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(chk)
    return chk, _lib.LIB_PATH


def kernel_instructions(text, name):
    """[(address, instruction text)] of the one kernel whose symbol holds `name`."""
    out, on, seen = [], False, 0
    for ln in text.splitlines():
        m = re.match(r"^[0-9a-f]+ <(.+)>:", ln)
        if m:
            on = name in m.group(1)
            seen += on
            continue
        if not on:
            continue
        t = ln.strip().split("//")[0].strip()
        a = re.search(r"//\s*([0-9A-Fa-f]{8,16}):", ln)
        if t and a:
            out.append((int(a.group(1), 16), t))
    assert seen == 1, f"{seen} kernels named *{name}* in the disassembly"
    return out


def natural_loops(ins):
    """Natural loops of the instruction-level control-flow graph: one set of instruction indices per loop header (the
    loops of the back edges into one header are merged).  A back edge is an edge whose target dominates its source."""
    n = len(ins)
    index = {a: i for i, (a, _) in enumerate(ins)}
    succ = [[] for _ in range(n)]
    for i, (a, t) in enumerate(ins):
        m = _BRANCH.match(t)
        if t.startswith(("s_endpgm", "s_setpc")):
            continue
        if m:
            off = int(m.group(2))
            off = off - 65536 if off >= 32768 else off
            tgt = index.get(a + 4 + 4 * off)
            assert tgt is not None, f"branch to an unknown address: {t}"
            succ[i].append(tgt)
            if m.group(1) == "branch":
                continue
        if i + 1 < n:
            succ[i].append(i + 1)
    # basic blocks
    leader = [False] * n
    leader[0] = True
    for i in range(n):
        if len(succ[i]) != 1 or succ[i][0] != i + 1:
            for s in succ[i]:
                leader[s] = True
            if i + 1 < n:
                leader[i + 1] = True
    starts = [i for i in range(n) if leader[i]]
    block_of = {}
    blocks = []
    for b, s in enumerate(starts):
        e = starts[b + 1] if b + 1 < len(starts) else n
        blocks.append(range(s, e))
        for i in range(s, e):
            block_of[i] = b
    nb = len(blocks)
    bsucc = [sorted({block_of[s] for s in succ[blk[-1]]}) for blk in blocks]
    bpred = [[] for _ in range(nb)]
    for b in range(nb):
        for s in bsucc[b]:
            bpred[s].append(b)
    # dominators (iterative, over a reverse post-order from the entry block)
    order, state, stack = [], [0] * nb, [(0, 0)]
    state[0] = 1
    while stack:
        b, k = stack.pop()
        if k < len(bsucc[b]):
            stack.append((b, k + 1))
            s = bsucc[b][k]
            if not state[s]:
                state[s] = 1
                stack.append((s, 0))
        else:
            order.append(b)
    rpo = order[::-1]
    pos = {b: k for k, b in enumerate(rpo)}
    idom = {0: 0}
    changed = True
    while changed:
        changed = False
        for b in rpo[1:]:
            new = None
            for p in bpred[b]:
                if p not in idom:
                    continue
                if new is None:
                    new = p
                    continue
                x, y = p, new
                while x != y:
                    while pos[x] > pos[y]:
                        x = idom[x]
                    while pos[y] > pos[x]:
                        y = idom[y]
                new = x
            if new is not None and idom.get(b) != new:
                idom[b] = new
                changed = True

    def dominates(h, b):
        while True:
            if b == h:
                return True
            if b == 0 or b not in idom:
                return False
            b = idom[b]

    loops = {}
    for b in range(nb):
        if b not in idom:
            continue
        for h in bsucc[b]:
            if dominates(h, b):
                body = loops.setdefault(h, {h})
                work = [b]
                while work:
                    x = work.pop()
                    if x not in body:
                        body.add(x)
                        work.extend(bpred[x])
    return [sorted(i for b in body for i in blocks[b]) for body in loops.values()]


def sample_loops(ins, reads=36):
    """The innermost loops that hold exactly `reads` ds_read_b64, as lists of instruction texts in address order."""
    loops = [set(l) for l in natural_loops(ins)]
    out = []
    for l in loops:
        if sum(1 for i in l if ins[i][1].startswith("ds_read_b64")) != reads:
            continue
        if any(o < l for o in loops):  # (holds another loop: not innermost)
            continue
        out.append([ins[i][1] for i in sorted(l)])
    return out


def _sregs(tok):
    out = set()
    for m in re.finditer(r"\bs\[(\d+):(\d+)\]", tok):
        out.update(range(int(m.group(1)), int(m.group(2)) + 1))
    for m in re.finditer(r"\bs(\d+)\b", tok):
        out.add(int(m.group(1)))
    return out


def point_address_instructions(body):
    """The scalar instructions of one loop iteration that the address of an `s_load_dwordx8` depends on: from each load,
    backwards round the loop to the nearest instruction that writes a register of its address pair, and on from there
    through that instruction's own scalar sources.  A register nothing in the loop writes is loop-invariant."""
    n = len(body)

    def ops(t):
        return [o.strip() for o in t.split(None, 1)[1].split(",")] if " " in t else []

    def writes(t):
        if not t.startswith("s_") or t.startswith(("s_waitcnt", "s_nop", "s_cmp", "s_cbranch", "s_branch", "s_bitcmp")):
            return set()
        o = ops(t)
        return _sregs(o[0]) if o else set()

    found, work = set(), []
    for i, t in enumerate(body):
        if t.startswith("s_load_dwordx8"):
            work.extend((i, r) for r in _sregs(ops(t)[1]))
    seen = set()
    while work:
        at, reg = work.pop()
        if (at, reg) in seen:
            continue
        seen.add((at, reg))
        for step in range(1, n + 1):
            k = (at - step) % n
            if reg in writes(body[k]):
                if not body[k].startswith("s_load"):
                    if k not in found:
                        found.add(k)
                    for o in ops(body[k])[1:]:
                        work.extend((k, r) for r in _sregs(o))
                break
    return [body[k] for k in sorted(found)]


def loop_table(body):
    valu = sum(1 for t in body if t.startswith("v_"))
    return {
        "valu": valu,
        "ds_read_b64": sum(1 for t in body if t.startswith("ds_read_b64")),
        "scalar": sum(1 for t in body if t.startswith("s_")),
        "s_nop": sum(1 for t in body if t.startswith("s_nop")),
        "lgkm0": sum(1 for t in body if t.startswith("s_waitcnt") and "lgkmcnt(0)" in t),
        "s_load_dwordx8": sum(1 for t in body if t.startswith("s_load_dwordx8")),
        "v_cmp": sum(1 for t in body if t.startswith("v_cmp")),
        "address": point_address_instructions(body),
    }


def classify(tables):
    """{'clean', 'masked', 'bounded'} -> table: CLEAN evaluates no sample mask (no v_cmp), the masked interior loop one
    v_cmp_class per sample, the bounded loop the bounds rule on top of it."""
    by = sorted(tables, key=lambda t: t["v_cmp"])
    assert len(by) == 3, f"{len(by)} sample loops of 36 reads in the headline kernel, expected 3"
    assert by[0]["v_cmp"] == 0 and by[1]["v_cmp"] == 4 and by[2]["v_cmp"] > 4, [t["v_cmp"] for t in by]
    return {"clean": by[0], "masked": by[1], "bounded": by[2]}


@pytest.fixture(scope="module")
def headline_loops():
    if not (os.path.exists(os.path.join(LLVM, "llvm-objdump")) and
            os.path.exists(os.path.join(LLVM, "clang-offload-bundler"))):
        pytest.skip("ROCm LLVM tools not installed")
    chk, lib = _check_isa()
    ins = kernel_instructions(chk.disassemble(lib), HEADLINE)
    loops = classify([loop_table(b) for b in sample_loops(ins)])
    for name, t in loops.items():
        print(name, {k: v for k, v in t.items()})
    return loops


def test_loop_finder_on_a_hand_made_listing():
    """The finder itself: a loop whose cold block lies before its header (as the compiler lays out the masked loop) is one
    loop with that block in it, and the outer loop round it is not innermost."""
    def line(addr, text):
        return f"\t{text}  // {addr:012X}: 00000000"
    rows = ["v_mov_b32 v0, 0",                  # 0x00 entry
            "s_branch 2",                       # 0x04 -> 0x10 (header)
            "v_add_u32 v1, 1, v1",              # 0x08 cold block of the loop, laid out before the header
            "s_branch 2",                       # 0x0c -> 0x18
            "ds_read_b64 v[2:3], v0",           # 0x10 header
            "s_cbranch_execz 65531",            # 0x14 -> 0x08 (into the cold block), else falls to 0x18
            "s_add_u32 s4, s4, 0x200",          # 0x18
            "s_cbranch_scc1 65532",             # 0x1c -> 0x10 back edge
            "s_cbranch_scc0 65528",             # 0x20 -> 0x04 outer back edge
            "s_endpgm"]
    text = "0000000000000000 <k>:\n" + "\n".join(line(4 * k, t) for k, t in enumerate(rows)) + "\n"
    ins = kernel_instructions(text, "k")
    inner = sample_loops(ins, reads=1)
    assert len(inner) == 1 and inner[0] == rows[2:8]
    assert point_address_instructions(["s_add_u32 s4, s4, 0x200", "s_addc_u32 s5, s5, 0",
                                       "s_load_dwordx8 s[8:15], s[4:5], 0x20", "s_add_i32 s6, s6, 4",
                                       "s_cmp_lt_u32 s6, s7"]) == ["s_add_u32 s4, s4, 0x200", "s_addc_u32 s5, s5, 0"]


@pytest.mark.parametrize("loop", ["masked", "clean", "bounded"])
def test_sample_loop_has_no_s_nop(headline_loops, loop):
    t = headline_loops[loop]
    assert t["ds_read_b64"] == 36 and t["s_load_dwordx8"] == 4
    assert t["s_nop"] == 0, t


@pytest.mark.parametrize("loop", ["masked", "clean", "bounded"])
def test_sample_loop_spends_at_most_two_scalar_instructions_on_the_point_address(headline_loops, loop):
    t = headline_loops[loop]
    assert len(t["address"]) <= 2, t["address"]


@pytest.mark.parametrize("loop", ["masked", "clean"])
def test_interior_loop_waits_once_per_gather(headline_loops, loop):
    assert headline_loops[loop]["lgkm0"] == 4, headline_loops[loop]


@pytest.mark.parametrize("loop,valu", [("masked", 140), ("clean", 127), ("bounded", 156)])
def test_sample_loop_vector_instruction_count(headline_loops, loop, valu):
    assert headline_loops[loop]["valu"] == valu, headline_loops[loop]
