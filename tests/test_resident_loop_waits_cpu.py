"""CPU: the resident kernel's iteration loop AS COMPILED ("the loop as compiled").

The builds that copy the inserted offsets in their loop exist in two forms (nlspn_resident.h
prop_resident_kernel COPY): with the copy, and the helper launch's, which holds no copy code
(template argument COPY = false, the last one of the mangled name).  While one loop served both,
the copy's load was statically pending in the registers the poison and the accumulators reuse,
and the compiler covered it with `s_waitcnt vmcnt(0)` at the loop header and right behind the
poison store: a launch that copied nothing waited there for its own stores' acknowledgements.

For the 3x3 builds of the bench shapes (C2's, the GROUPS build, their fp16 twins) the no-copy
loop of the device assembly must have
  * no s_waitcnt with a vmcnt field between a poison store and the first tap read (ds_read_b64),
  * no vmcnt wait between the loop header and the first sc1 staging load (the t >= 2 path: the
    iteration-1 placement poll sits in inner loops of its own and is not on it),
  * the explicit vmcnt(0) in front of the plane store (the hand-off's ordering rule) still there.
The loops are found by the poison constant.  The wide unit (1x17, 5x5) is inspected by hand
(DESIGN.md): compiling it here too would double the test's time.
"""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "nlspn_eccv20_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
# the Makefile's flags for the resident units, as tests/test_resource_usage_cpu.py has them
_FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-slp-vectorize"]
POISON = ("0x7f800bad", "0x7d0b7d0b")  # kPoison32; kPoison16 in both halves of a dword

# <T, 3, 3, 768, 1, 576, GROUPS, FIRST = true, PXO = 0, COPY = false>
_KERNEL = "_ZN5nlspn20prop_resident_kernelI%sLi3ELi3ELi768ELi1ELi576ELb%dELb1ELi0ELb0EEEvNS_7ResArgsE"
BUILDS = {  # name: (mangled name, depth of the iteration loop: the GROUPS builds nest it in the group loop)
    "c2_f32": (_KERNEL % ("f", 0), 1),
    "groups_f32": (_KERNEL % ("f", 1), 2),
    "c2_f16": (_KERNEL % ("6__half", 0), 1),
    "groups_f16": (_KERNEL % ("6__half", 1), 2),
}

_LABEL = re.compile(r"^(?:\.L(BB\d+_\d+):|; %bb\.\d+:)")
_VMWAIT = re.compile(r"^\s*s_waitcnt\b.*\bvmcnt\(")
_NT_STORE = re.compile(r"^\s*buffer_store_\S+ .*\bnt\b")
_STAGE_LOAD = re.compile(r"^\s*buffer_load_dwordx[24] .*\bsc1\b")
_TAP_READ = re.compile(r"^\s*ds_read_b64\b")


def kernel_body(asm, name):
    i = asm.index("\n" + name + ":")
    return asm[i:asm.index(".Lfunc_end", i)].splitlines()


def blocks(lines):
    """Basic blocks in layout order: {"label", "loop" (innermost loop's header label or None),
    "depth", "parents" (a header's enclosing loops), "lines"}, from LLVM's block comments
    (`in Loop: Header=BBn_m Depth=D`, `Parent Loop BBn_m Depth=D`, `=>This Loop Header: Depth=D`)."""
    out, cur, in_comment = [], None, False
    for ln in lines:
        m = _LABEL.match(ln)
        if m:
            cur = {"label": m.group(1), "loop": None, "depth": 0, "parents": [], "lines": []}
            out.append(cur)
            in_comment = True
        elif cur is None:
            continue
        elif not (in_comment and re.match(r"^\s+;.*Loop", ln)):
            in_comment = False
            cur["lines"].append(ln)
            continue
        c = ln.split(";", 1)[1] if ";" in ln else ""
        m = re.search(r"in Loop: Header=(BB\d+_\d+) Depth=(\d+)", c)
        if m:
            cur["loop"], cur["depth"] = m.group(1), int(m.group(2))
        m = re.search(r"Parent Loop (BB\d+_\d+) Depth=\d+", c)
        if m:
            cur["parents"].append(m.group(1))
        m = re.search(r"This (?:Inner )?Loop Header: Depth=(\d+)", c)
        if m:
            cur["loop"], cur["depth"] = cur["label"], int(m.group(1))
    return out


def _has_poison_store(b):
    at = [i for i, ln in enumerate(b["lines"]) if re.match(r"^\s*v_mov_b32\S* v\d+, (%s)\b" % "|".join(POISON), ln)]
    return any(re.match(r"^\s*buffer_store_", ln) for i in at for ln in b["lines"][i:])


def iteration_loops(bl, depth):
    """The loops at `depth` that store the poison in a block of their own level, in layout order:
    [{"header", "copy" (streaming stores inside: the inserted-offset copy), "blocks"}]."""
    parents = {b["label"]: b["parents"] for b in bl if b["loop"] == b["label"]}
    heads = [b["loop"] for b in bl if b["depth"] == depth and _has_poison_store(b)]
    out = []
    for h in dict.fromkeys(heads):
        mine = [b for b in bl if b["loop"] == h or h in parents.get(b["loop"], [])]
        out.append({"header": h, "blocks": mine,
                    "copy": any(_NT_STORE.match(ln) for b in mine for ln in b["lines"])})
    return out


def waits_after_poison(loop):
    """Per poison store: the vmcnt waits from the store to the first tap read, in layout order."""
    flat = [ln for b in loop["blocks"] for ln in b["lines"]]
    blk = [n for n, b in enumerate(loop["blocks"]) for _ in b["lines"]]
    found = []
    for i, ln in enumerate(flat):
        if not re.match(r"^\s*v_mov_b32\S* v\d+, (%s)\b" % "|".join(POISON), ln):
            continue
        st = next((j for j in range(i, len(flat)) if re.match(r"^\s*buffer_store_", flat[j])), None)
        if st is None or blk[st] != blk[i]:
            continue  # (a compare's constant, not a store's)
        rd = next((j for j in range(st, len(flat)) if _TAP_READ.match(flat[j])), None)
        assert rd is not None, "no tap read behind a poison store"
        found.append([x.strip() for x in flat[st:rd] if _VMWAIT.match(x)])
    return found


def waits_before_staging(loop):
    """The vmcnt waits from the loop header to the first sc1 staging load: the loop's own-level
    blocks up to the staging loop (the first inner loop holding such a load), then that loop from
    its header to the load."""
    h = loop["header"]
    stage = next(b["loop"] for b in loop["blocks"] if b["loop"] != h and any(_STAGE_LOAD.match(x) for x in b["lines"]))
    labels = [b["label"] for b in loop["blocks"]]
    i0, i1 = labels.index(h), labels.index(stage)
    assert i0 < i1, "the staging loop lies before the loop header"
    waits = [x.strip() for b in loop["blocks"][i0:i1] if b["loop"] == h for x in b["lines"] if _VMWAIT.match(x)]
    for b in loop["blocks"][i1:]:
        if b["loop"] != stage:
            continue
        for x in b["lines"]:
            if _STAGE_LOAD.match(x):
                return waits
            if _VMWAIT.match(x):
                waits.append(x.strip())
    raise AssertionError("no staging load in the staging loop")


def explicit_prestore_wait(loop):
    """The source's own `s_waitcnt vmcnt(0)` (inline assembly) between the tap reads and a store
    (the plane's) behind it in the loop."""
    flat = [ln.strip() for b in loop["blocks"] for ln in b["lines"]]
    for i in range(len(flat) - 2):
        if flat[i].startswith(";;#ASMSTART") and flat[i + 1] == "s_waitcnt vmcnt(0)" and flat[i + 2].startswith(";;#ASMEND"):
            if any(_TAP_READ.match(x) for x in flat[:i]) and any(x.startswith("buffer_store_") for x in flat[i + 3:]):
                return True
    return False


# ---- the parser on literal snippets

_SNIP = """
_Zk:
; %bb.0:
	s_waitcnt vmcnt(0)
.LBB0_1:                                ; =>This Loop Header: Depth=1
                                        ;     Child Loop BB0_3 Depth 2
	v_mov_b32_e32 v1, 0
; %bb.2:                                ;   in Loop: Header=BB0_1 Depth=1
	{HEADWAIT}
.LBB0_3:                                ;   Parent Loop BB0_1 Depth=1
                                        ; =>  This Inner Loop Header: Depth=2
	buffer_load_dwordx4 v[4:7], v2, s[4:7], 0 offen sc1
	s_waitcnt vmcnt(0)
	s_cbranch_execnz .LBB0_3
; %bb.4:                                ;   in Loop: Header=BB0_1 Depth=1
	s_barrier
	v_mov_b32_e32 v12, 0x7f800bad
	buffer_store_dwordx4 v[12:15], v3, s[8:11], 0 offen sc1
.LBB0_5:                                ;   in Loop: Header=BB0_1 Depth=1
	{POSTWAIT}
	ds_read_b64 v[2:3], v1
	;;#ASMSTART
	s_waitcnt vmcnt(0)
	;;#ASMEND
	buffer_store_dwordx4 v[16:19], v3, s[8:11], 0 offen sc1
	{COPY}
	s_cbranch_scc0 .LBB0_1
; %bb.6:
	s_endpgm
.Lfunc_end0:
"""


def _snip(head="s_nop 0", post="s_nop 0", copy="s_nop 0"):
    return blocks(kernel_body(_SNIP.format(HEADWAIT=head, POSTWAIT=post, COPY=copy), "_Zk"))


def test_parser_blocks_and_loops():
    bl = _snip()
    assert [b["label"] for b in bl] == [None, "BB0_1", None, "BB0_3", None, "BB0_5", None]
    assert [(b["loop"], b["depth"]) for b in bl] == [(None, 0), ("BB0_1", 1), ("BB0_1", 1), ("BB0_3", 2),
                                                    ("BB0_1", 1), ("BB0_1", 1), (None, 0)]
    assert bl[3]["parents"] == ["BB0_1"]
    (loop,) = iteration_loops(bl, 1)
    assert loop["header"] == "BB0_1" and not loop["copy"] and len(loop["blocks"]) == 5
    assert iteration_loops(bl, 2) == []
    assert waits_after_poison(loop) == [[]] and waits_before_staging(loop) == [] and explicit_prestore_wait(loop)


def test_parser_finds_the_waits():
    (loop,) = iteration_loops(_snip(head="s_waitcnt vmcnt(0)", post="s_waitcnt vmcnt(1) lgkmcnt(0)"), 1)
    assert waits_before_staging(loop) == ["s_waitcnt vmcnt(0)"]
    assert waits_after_poison(loop) == [["s_waitcnt vmcnt(1) lgkmcnt(0)"]]
    (loop,) = iteration_loops(_snip(post="s_waitcnt lgkmcnt(0)"), 1)  # no vmcnt field: not counted
    assert waits_after_poison(loop) == [[]]
    (loop,) = iteration_loops(_snip(copy="buffer_store_dwordx4 v[4:7], v3, s[12:15], s2 offen nt"), 1)
    assert loop["copy"]


# ---- the compiled loop

@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    if not (os.path.exists(HIPCC) or shutil.which("hipcc")):
        pytest.skip("hipcc missing")
    path = str(tmp_path_factory.mktemp("resloop") / "nlspn_kern_resident.s")
    out = subprocess.run([HIPCC if os.path.exists(HIPCC) else "hipcc", *_FLAGS, "--cuda-device-only", "-S", "-o", path,
                          os.path.join(CSRC, "nlspn_kern_resident.hip")], capture_output=True, text=True, cwd=CSRC)
    assert out.returncode == 0, out.stderr[-2000:]
    with open(path) as f:
        return f.read()


@pytest.mark.parametrize("build", sorted(BUILDS))
def test_no_copy_loop_waits_for_no_store(asm, build):
    name, depth = BUILDS[build]
    if "\n" + name + ":" not in asm:  # one loop form only: say what it waits for
        one = name.replace("ELi0ELb0EEE", "ELi0EEE")
        seen = {}
        if "\n" + one + ":" in asm:
            seen = {lp["header"]: {"before staging": waits_before_staging(lp), "after poison": waits_after_poison(lp)}
                    for lp in iteration_loops(blocks(kernel_body(asm, one)), depth)}
        pytest.fail(f"no build without the loop's copy code (COPY = false) in the unit; the one loop form waits: {seen}")
    loops = iteration_loops(blocks(kernel_body(asm, name)), depth)
    assert loops, "no iteration loop found by the poison constant"
    plain = [lp for lp in loops if not lp["copy"]]
    seen = {lp["header"]: (waits_before_staging(lp), waits_after_poison(lp)) for lp in loops}
    print(build, seen)
    assert len(plain) == 1 and len(loops) == 1, f"expected one iteration loop, without copy code: {seen}"
    head, post = seen[plain[0]["header"]]
    assert post and all(w == [] for w in post), f"vmcnt waits between a poison store and the first tap read: {post}"
    assert head == [], f"vmcnt waits between the loop header and the first sc1 staging load: {head}"
    assert explicit_prestore_wait(plain[0]), "the explicit wait in front of the plane store is gone"
