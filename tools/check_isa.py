#!/usr/bin/env python3
"""Guards on the resident FFT kernel's code object (run on CPU; tests/test_abi_cpu.py calls it).

The kernel (opencl_fft_amd/csrc/fft_resident.hip, one translation unit with its fft_res_*.inc) does two things hipcc cannot check:
  * it manages the accumulation register file by hand (literal a[N] in inline asm), so the compiler
    must not place anything of its own there: no v_accvgpr_* outside the asm blocks, no scratch;
  * it issues global loads from inline asm (hipcc neither counts nor waits for them) into AGPRs and
    into v[224:255], which amdgpu_num_vgpr(224) keeps out of the register allocator's hands: no
    compiler-generated instruction may name those registers (with compiler-allocated destinations
    hipcc was seen copying them ahead of the kernel's own s_waitcnt, i.e. before the data had landed).

usage: check_isa.py file.s                (hipcc -save-temps of fft_resident.hip)
       check_isa.py --handover a.s b.s   (pconv_coop.hip and dconv_block.hip: the inter-workgroup hand-overs of handover.hpp)
       check_isa.py --same OLD.s NEW.s    (a refactor's proof: every kernel compiles to the instructions it had)
"""
import re
import sys

REG = re.compile(r"\bv(\d+)\b|\bv\[(\d+):(\d+)\]")
AREG = re.compile(r"\ba(\d+)\b|\ba\[(\d+):(\d+)\]")
RESERVED_FIRST = 224   # v[224:255]: landing registers of asm-issued loads (kernel built with amdgpu_num_vgpr(224))


def regs_of(text):
    out = set()
    for m in REG.finditer(text):
        if m.group(1) is not None:
            out.add(int(m.group(1)))
        else:
            out.update(range(int(m.group(2)), int(m.group(3)) + 1))
    return out


def audit_reserved(body):
    """no instruction outside the kernel's own asm statements may name a reserved VGPR"""
    problems = []
    inasm = False
    for ln in body.split("\n"):
        s = ln.strip()
        if "ASMSTART" in s:
            inasm = True
            continue
        if "ASMEND" in s:
            inasm = False
            continue
        if inasm or not s or s.startswith((";", ".")):
            continue
        code = s.split(";")[0]
        hit = [r for r in regs_of(code) if r >= RESERVED_FIRST]
        if hit:
            problems.append("compiler instruction touches reserved v%s: %s" % (sorted(hit), code.strip()))
        # on gfx90a+ the allocator may name an AGPR directly as an operand (AV register class: ds_*, buffer_*,
        # v_mov ...) without any v_accvgpr_* instruction: the whole accumulation file is the kernel's own
        if AREG.search(code.split(None, 1)[1] if " " in code.strip() or "\t" in code.strip() else ""):
            problems.append("compiler instruction names an AGPR: %s" % code.strip())
    return problems


def audit_loop_loads(body):
    """the explicit s_waitcnt vmcnt(N) scheme counts the asm-issued loads only: a compiler-issued global / buffer
    LOAD anywhere after the table prologue would shift every count.  Compiler-issued stores only make a wait
    stronger and are allowed (the slot's write-through store, the last block's burst)."""
    problems = []
    inasm = False
    seen_barrier = False
    for ln in body.split("\n"):
        s = ln.strip()
        if "ASMSTART" in s:
            inasm = True
            continue
        if "ASMEND" in s:
            inasm = False
            continue
        if inasm or not s or s.startswith((";", ".")):
            continue
        code = s.split(";")[0].strip()
        if code.startswith("s_barrier"):
            seen_barrier = True
        if seen_barrier and re.match(r"(buffer|global|flat)_load", code):
            problems.append("compiler-issued vector load behind the prologue: %s" % code)
    return problems


def metadata_of(s, name):
    """.amdhsa / amdhsa.kernels metadata of one kernel -> dict of the integer fields"""
    m = re.search(r"- \.agpr_count:.*?\.name:\s+%s\b.*?(?=\n  - \.agpr_count:|\n\.\.\.|\Z)" % re.escape(name), s, re.S)
    out = {}
    if m:
        for k, v in re.findall(r"\.(\w+):\s+(\d+)\s*$", m.group(0), re.M):
            out[k] = int(v)
    return out


def check(path):
    s = open(path).read()
    problems = []
    found = 0
    for m in re.finditer(r"^(_ZN4clfa11k_fft_res16[A-Za-z0-9_]+):", s, re.M):
        found += 1
        name = m.group(1)
        body = s[m.end():]
        body = body[:body.index(".Lfunc_end")]
        inasm = False
        stray = 0
        for ln in body.split("\n"):
            if "ASMSTART" in ln:
                inasm = True
            elif "ASMEND" in ln:
                inasm = False
            elif "accvgpr" in ln and not inasm:
                stray += 1
        if stray:
            problems.append("%s: %d compiler-generated AGPR moves" % (name, stray))
        if re.search(r"\bscratch_(load|store)", body):
            problems.append("%s: scratch memory accesses" % name)
        for p in audit_reserved(body) + audit_loop_loads(body):
            problems.append("%s: %s" % (name, p))
        md = metadata_of(s, name)
        if not md:
            problems.append("%s: no kernel metadata found" % name)
        else:
            for key in ("private_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count"):
                if md.get(key, 0) != 0:
                    problems.append("%s: %s = %d" % (name, key, md[key]))
    if not found:
        problems.append("no k_fft_res16 kernel in %s" % path)
    return problems


def check_handover(*paths):
    """pconv_coop.hip + dconv_block.hip (handover.hpp), one .s file each, read as one text: the inter-workgroup hand-overs
    of k_pconv_coop / k_dconv_block read the handed-over bytes with
    agent-scope loads that must compile to global_ / buffer_ loads with sc1 (never flat_: MI355X_MICROARCH.md, 'Valid
    forms', Consumer bullet), store them with sc1 stores, drain with s_waitcnt vmcnt(0) in front of the arrival add (which
    is an agent-scope RELEASE in the C++ model as well), and —
    for launches with more workgroups than CUs — carry an agent-scope acquire (buffer_inv sc1) for the last workgroup."""
    s = "\n".join(open(p).read() for p in paths)
    path = " + ".join(paths)
    problems = []
    for stem, least_loads in (("k_pconv_coop", 2), ("k_dconv_block", 8)):
        names = re.findall(r"^(_ZN4clfa\d+%s[A-Za-z0-9_]*):" % stem, s, re.M)
        if not names:
            problems.append("no %s kernel in %s" % (stem, path))
        for name in names:
            body = s[s.index("\n" + name + ":"):]
            body = body[:body.index(".Lfunc_end")]
            code = [ln.split(";")[0].strip() for ln in body.split("\n")]
            sc1_loads = [c for c in code if re.match(r"(global|buffer|flat|scratch)_load\S*\s.*\bsc1\b", c)]
            if len(sc1_loads) < least_loads:
                problems.append("%s: %d agent-scope (sc1) loads, expected at least %d" % (name, len(sc1_loads), least_loads))
            for c in sc1_loads:
                if not c.startswith(("global_load", "buffer_load")):
                    problems.append("%s: agent-scope load is not a global_/buffer_ load: %s" % (name, c))
            if any(re.match(r"flat_(load|store|atomic)", c) for c in code):
                problems.append("%s: flat_ memory instruction in a hand-over kernel" % name)
            if not any(re.match(r"(global|buffer)_store\S*\s.*\bsc1\b", c) for c in code):
                problems.append("%s: no sc1 (write-through) store of the handed-over bytes" % name)
            if not any(re.match(r"(global|buffer)_atomic_add\S*\s.*\bsc0\b", c) or re.match(r"(global|buffer)_atomic_add", c) for c in code):
                problems.append("%s: no arrival counter add" % name)
            # the arrival add carries an agent-scope release (handover.hpp, handover_arrive): a write-back and its wait
            # directly in front of every counter add
            adds = [i for i, c in enumerate(code) if re.match(r"(global|buffer)_atomic_add", c)]
            for i in adds:
                before = [c for c in code[max(0, i - 6):i] if c]
                if not any(c.startswith("buffer_wbl2") and "sc1" in c for c in before) or not any(c.startswith("s_waitcnt") and "vmcnt(0)" in c for c in before):
                    problems.append("%s: counter add without an agent-scope release (buffer_wbl2 sc1 + s_waitcnt vmcnt(0)) in front of it" % name)
            if not any(c.startswith("buffer_inv") and "sc1" in c for c in code):
                problems.append("%s: no agent-scope acquire (buffer_inv sc1) for launches beyond one workgroup per CU" % name)
    return problems


def kernels_of(path):
    """kernel symbol -> (basic blocks, .amdhsa_ descriptor lines) of a hipcc -save-temps .s file: comments, .loc / .file /
    .ident / .section directives dropped, local labels renumbered in order of appearance"""
    s = open(path).read()
    out = {}
    for m in re.finditer(r"^(_ZN4clfa\w+):.*?\n(.*?)^\.Lfunc_end\d+:", s, re.S | re.M):
        code, desc, labels, in_desc = [[]], [], {}, False
        for ln in m.group(2).split("\n"):
            if "; %bb." in ln:
                code.append([])   # a block the assembly falls into has no label of its own
            t = ln.split(";")[0].strip()
            if t.startswith(".amdhsa_kernel") or t.startswith(".end_amdhsa_kernel"):
                in_desc = not in_desc
            elif in_desc:
                desc.append(" ".join(t.split()))
            elif t and not t.startswith((".loc", ".file", ".ident", ".section", ".p2align", ".cfi")):
                t = re.sub(r"\.L\w+", lambda l: labels.setdefault(l.group(0), ".L%d" % len(labels)), " ".join(t.split()))
                if t.endswith(":"):
                    code.append([])
                code[-1].append(t)
        out[m.group(1)] = ([b for b in code if b], desc)
    return out


def same(old, new, out=sys.stdout):
    """one line per kernel: name, instructions, same / reordered / DIFFERENT.  `reordered`: the descriptor (register
    counts, LDS, scratch) is equal and every basic block holds the same instructions in another order; its diff is
    printed and has to be READ: the multiset rule also passes a swap of two dependent instructions, and only a person
    can tell that the moved ones are independent.  Returns the number of kernels that are DIFFERENT, missing or new
    (a `reordered` kernel does not count: the exit status alone is no proof of identity)."""
    import difflib
    a, b = kernels_of(old), kernels_of(new)
    bad = 0
    for name in sorted(set(a) | set(b)):
        if name not in a or name not in b:
            print("%s  -  %s" % (name, "MISSING in new" if name in a else "NEW kernel"), file=out)
            bad += 1
            continue
        (ca, da), (cb, db) = a[name], b[name]
        n = sum(not t.startswith(".") for blk in cb for t in blk)   # labels and directives are compared, not counted
        if (ca, da) == (cb, db):
            verdict = "same"
        elif da == db and len(ca) == len(cb) and all(sorted(x) == sorted(y) for x, y in zip(ca, cb)):
            verdict = "reordered"
        else:
            verdict = "DIFFERENT"
            bad += 1
        print("%s  %d  %s" % (name, n, verdict), file=out)
        if verdict != "same":
            flat = lambda c, d: [t for blk in c for t in blk] + d
            for ln in list(difflib.unified_diff(flat(ca, da), flat(cb, db), "old", "new", n=1, lineterm=""))[:80]:
                print("    " + ln, file=out)
    return bad


if __name__ == "__main__":
    if len(sys.argv) > 3 and sys.argv[1] == "--same":
        sys.exit(1 if same(sys.argv[2], sys.argv[3]) else 0)
    if len(sys.argv) > 2 and sys.argv[1] == "--handover":
        p = check_handover(*sys.argv[2:])
        for x in p:
            print(x)
        sys.exit(1 if p else 0)
    p = check(sys.argv[1])
    for x in p:
        print(x)
    sys.exit(1 if p else 0)
