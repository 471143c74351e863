"""Static check of the gfx950 device code: cross-workgroup hand-overs are ordered on every control-flow path.

The merged weight-gradient launch hands K-slice slabs to the last-arriving workgroup of a tile: each slice writes
its slab with write-through (sc1) vector stores, then advances the tile's arrival counter with a vector atomic.
The reader may run on another XCD, so the counter may only move once every slab store of the writing workgroup
has been acknowledged, i.e. after an ``s_waitcnt`` that drains vmcnt.  A race window of this kind is too narrow for
parity tests to catch, so it is pinned in the ISA: every ``.hip`` file of the library is compiled to device
assembly with the library's flags, and for every function no path of its control-flow graph (labels, branch
targets, fall-through; loops included) may lead from an sc1 vector store to a vector atomic without passing an
``s_waitcnt`` whose vmcnt is 0.  Scanning the text in file order is not enough: a wait a few lines above the
atomic can sit in a branch arm that the store's path jumps over.
"""
import os
import re
import shutil
import subprocess
from concurrent.futures import ThreadPoolExecutor

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "st-dadk_amd", "csrc")

_VSTORE = re.compile(r"^(global|buffer|flat)_store\w*$")
_VATOMIC = re.compile(r"^(global|buffer|flat)_atomic\w*$")
_LABEL = re.compile(r"^([.\w$]+):")
_FUNC_TYPE = re.compile(r"^\s*\.type\s+([\w.$]+)\s*,\s*@function", re.M)


def _hipcc():
    cand = os.environ.get("HIPCC") or "/opt/rocm/bin/hipcc"
    if os.path.exists(cand):
        return cand
    return shutil.which("hipcc")


def _build_flags():
    """The FLAGS line of build.sh (so the checked code is the shipped code), minus the shell expansion."""
    text = open(os.path.join(CSRC, "build.sh")).read()
    m = re.search(r'^FLAGS="([^"]*)"', text, flags=re.M)
    assert m, "FLAGS= line not found in build.sh"
    return [f for f in m.group(1).split() if not f.startswith("${")]


def _waits_vm0(operands):
    """True for an s_waitcnt that drains the vector-memory counter: vmcnt(0) alone or beside other counters,
    or the all-zero immediate."""
    ops = operands.strip()
    if re.fullmatch(r"0|0x0", ops):
        return True
    return re.search(r"\bvmcnt\(0\)", ops) is not None


def _functions(asm):
    """{function name: [instruction or label lines]} of one assembly file."""
    names = set(_FUNC_TYPE.findall(asm))
    out, cur, body = {}, None, None
    for raw in asm.splitlines():
        line = raw.split(";", 1)[0].rstrip()
        m = _LABEL.match(line.strip())
        if m and m.group(1) in names:
            cur, body = m.group(1), []
            out[cur] = body
            continue
        if cur is None:
            continue
        s = line.strip()
        if not s:
            continue
        if m and m.group(1).startswith(".Lfunc_end"):
            cur = None
            continue
        if s.startswith(".") and not m:         # directives
            continue
        body.append(s)
    return out


def _blocks(lines):
    """Basic blocks: [(label or None, [(mnemonic, operands, text)], successors)]."""
    blocks, cur_label, cur = [], None, []

    def close():
        blocks.append([cur_label, cur])

    for s in lines:
        m = _LABEL.match(s)
        if m:
            if cur or cur_label is not None:
                close()
            cur_label, cur = m.group(1), []
            continue
        parts = s.split(None, 1)
        mn, ops = parts[0], (parts[1] if len(parts) > 1 else "")
        cur.append((mn, ops, s))
        if mn.startswith("s_branch") or mn.startswith("s_cbranch") or mn in ("s_endpgm", "s_setpc_b64"):
            close()
            cur_label, cur = None, []
    if cur or cur_label is not None:
        close()
    index = {b[0]: i for i, b in enumerate(blocks) if b[0] is not None}
    out = []
    for i, (label, ins) in enumerate(blocks):
        succ = []
        last = ins[-1] if ins else None
        if last is not None and last[0] == "s_branch":
            succ.append(index[last[1].strip()])
        elif last is not None and last[0] in ("s_endpgm", "s_setpc_b64"):
            pass
        else:
            if last is not None and last[0].startswith("s_cbranch"):
                succ.append(index[last[1].strip()])
            if i + 1 < len(blocks):
                succ.append(i + 1)
        out.append((label, ins, succ))
    return out


def unordered_handovers(lines):
    """[(store text, atomic text)] for every sc1 vector store from which some path reaches a vector atomic
    without an s_waitcnt that drains vmcnt.  Forward may-analysis over the CFG; the fact is the set of
    sc1 stores that may still be outstanding."""
    blocks = _blocks(lines)
    if not blocks:
        return []
    ins_state = [None] * len(blocks)
    ins_state[0] = frozenset()
    work = [0]
    found = set()
    while work:
        i = work.pop()
        pending = set(ins_state[i])
        _, ins, succ = blocks[i]
        for mn, ops, text in ins:
            if mn == "s_waitcnt" and _waits_vm0(ops):
                pending.clear()
            elif _VATOMIC.match(mn):
                for st in pending:
                    found.add((st, text))
            elif _VSTORE.match(mn) and re.search(r"\bsc1\b", ops):
                pending.add(text)
        for j in succ:
            new = frozenset(pending) if ins_state[j] is None else ins_state[j] | pending
            if new != ins_state[j]:
                ins_state[j] = new
                work.append(j)
    return sorted(found)


# ---- self-tests of the checker on hand-written shapes --------------------------------------------------------

_HEAD_SHAPE = """
	s_cbranch_scc1 .LBB0_2
	global_store_dword v[8:9], a15, off sc1
	s_branch .LBB0_3
.LBB0_2:
	s_mov_b64 s[0:1], -1
	s_waitcnt vmcnt(0)
	global_store_dword v[2:3], v4, off
.LBB0_3:
	s_waitcnt lgkmcnt(0)
	s_barrier
	global_atomic_add v2, v2, v3, s[2:3] sc0
	s_endpgm
"""

_JOIN_WAIT = """
	s_cbranch_scc1 .LBB0_2
	global_store_dword v[8:9], a15, off sc1
	s_branch .LBB0_3
.LBB0_2:
	global_store_dword v[2:3], v4, off
.LBB0_3:
	s_waitcnt vmcnt(0) lgkmcnt(0)
	s_barrier
	global_atomic_add v2, v2, v3, s[2:3] sc0
	s_endpgm
"""

_LOOP_SHAPE = """
	s_waitcnt vmcnt(0)
.LBB0_1:
	global_atomic_add v2, v2, v3, s[2:3] sc0
	global_store_dwordx4 v[8:9], v[4:7], off sc1
	s_cbranch_scc1 .LBB0_1
	s_endpgm
"""


def _lines(src):
    return [s.strip() for s in src.strip().splitlines() if s.strip()]


def test_checker_flags_store_in_branch_arm_that_jumps_past_the_wait():
    bad = unordered_handovers(_lines(_HEAD_SHAPE))
    assert bad == [("global_store_dword v[8:9], a15, off sc1", "global_atomic_add v2, v2, v3, s[2:3] sc0")]
    # a linear scan would see the vmcnt(0) between the store and the atomic and pass this shape
    text = _lines(_HEAD_SHAPE)
    assert any("vmcnt(0)" in t for t in text[text.index("global_store_dword v[8:9], a15, off sc1"):])


def test_checker_passes_a_wait_in_the_join_block():
    assert unordered_handovers(_lines(_JOIN_WAIT)) == []
    assert unordered_handovers(_lines(_JOIN_WAIT.replace("vmcnt(0) lgkmcnt(0)", "0"))) == []
    # a partial drain is no drain
    assert unordered_handovers(_lines(_JOIN_WAIT.replace("vmcnt(0) lgkmcnt(0)", "vmcnt(1) lgkmcnt(0)")))
    assert unordered_handovers(_lines(_JOIN_WAIT.replace("vmcnt(0) lgkmcnt(0)", "lgkmcnt(0)")))


def test_checker_follows_loop_back_edges():
    bad = unordered_handovers(_lines(_LOOP_SHAPE))
    assert bad == [("global_store_dwordx4 v[8:9], v[4:7], off sc1", "global_atomic_add v2, v2, v3, s[2:3] sc0")]
    # a wait inside the loop, ahead of the atomic, orders it
    fixed = _LOOP_SHAPE.replace(".LBB0_1:\n", ".LBB0_1:\n\ts_waitcnt vmcnt(0)\n")
    assert unordered_handovers(_lines(fixed)) == []


def test_checker_ignores_plain_stores_and_functions_split_by_directives():
    asm = """
	.type	_Zk1,@function
_Zk1:                                  ; @_Zk1
	global_store_dword v[2:3], v4, off
	global_atomic_add v2, v2, v3, s[2:3] sc0
	s_endpgm
.Lfunc_end0:
	.type	_Zk2,@function
_Zk2:
	buffer_store_dword v1, v2, s[4:7], 0 offen sc0 sc1
	flat_atomic_add v[0:1], v2
	s_setpc_b64 s[30:31]
.Lfunc_end1:
"""
    fns = _functions(asm)
    assert set(fns) == {"_Zk1", "_Zk2"}
    assert unordered_handovers(fns["_Zk1"]) == []
    assert unordered_handovers(fns["_Zk2"]) == [("buffer_store_dword v1, v2, s[4:7], 0 offen sc0 sc1",
                                                 "flat_atomic_add v[0:1], v2")]


# ---- the library ------------------------------------------------------------------------------------------------

def _compile(hipcc, flags, src, out):
    r = subprocess.run([hipcc, *flags, "--cuda-device-only", "-S", src, "-o", out], capture_output=True, text=True)
    return src, out, r.returncode, r.stderr


def test_cross_workgroup_handovers_are_ordered_on_every_path(tmp_path):
    hipcc = _hipcc()
    if hipcc is None:
        pytest.skip("hipcc not available")
    flags = _build_flags()
    srcs = sorted(f for f in os.listdir(CSRC) if f.endswith(".hip"))
    assert srcs
    jobs = [(os.path.join(CSRC, f), str(tmp_path / (f[:-4] + ".s"))) for f in srcs]
    with ThreadPoolExecutor(max_workers=min(16, len(jobs))) as ex:
        results = list(ex.map(lambda j: _compile(hipcc, flags, *j), jobs))
    failures = [f"{os.path.basename(s)}:\n{err[-2000:]}" for s, _, rc, err in results if rc != 0]
    assert not failures, "device compile failed:\n" + "\n".join(failures)
    bad, n_fn, n_sc1 = [], 0, 0
    for src, out, _, _ in results:
        for name, lines in _functions(open(out).read()).items():
            n_fn += 1
            n_sc1 += sum(1 for s in lines if _VSTORE.match(s.split(None, 1)[0]) and re.search(r"\bsc1\b", s))
            pairs = unordered_handovers(lines)
            if pairs:
                st, at = pairs[0]
                bad.append(f"{os.path.basename(src)}: {name}: '{st}' reaches '{at}' with no s_waitcnt vmcnt(0)"
                           f" ({len(pairs)} such store/atomic pairs)")
    assert n_fn > 0 and n_sc1 > 0, (n_fn, n_sc1)      # the parser saw the kernels and the slab stores
    assert not bad, f"{len(bad)} function(s) with unordered hand-overs:\n" + "\n".join(bad)
