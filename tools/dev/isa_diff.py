"""Kernel-by-kernel comparison of the gfx950 device code of two trees (dev tool; needs hipcc, no GPU).

    python tools/dev/isa_diff.py emit    <tree> <outdir> [unit.hip ...]  # one .s per translation unit (default: all), the build's own flags
    python tools/dev/isa_diff.py compare <parent .s dir> <new .s dir> [new-kernel-substring=parent-mangled-name ...]

A refactor that must not change device code is checked here instead of on a GPU: every kernel (symbol with an .amdhsa_kernel block)
of the new tree has to exist in the parent under the same mangled name - or under the parent instantiation given for it on the
command line, where template parameters were dropped - with identical instruction text (comments stripped, the kernel's own name
and the function index of local labels .LBB<n>_ replaced) and equal VGPR / SGPR / AGPR-offset / LDS / scratch figures.  The kernels
of ALL units of a tree are pooled, so a kernel may move to another translation unit; one that the new tree emits from more than one
unit is a defect.  A kernel that differs is reported as "class B" if it has the same number of instruction lines with the same
mnemonic (first token) on every line and equal descriptor figures, i.e. only operands changed.  Parent kernels that the new tree no
longer has are listed.  Exit status 1 if any surviving kernel differs (class B included), is duplicated or has no parent."""
import os, re, subprocess, sys

DESC = (".amdhsa_next_free_vgpr", ".amdhsa_next_free_sgpr", ".amdhsa_accum_offset", ".amdhsa_group_segment_fixed_size",
        ".amdhsa_private_segment_fixed_size")


def emit(tree, outdir, only):
    sys.path.insert(0, tree)
    from flowtrack.pytorch_amd import build as b          # SOURCES, FLAGS and ARCH of THAT tree
    os.makedirs(outdir, exist_ok=True)
    procs = []
    for src in only or b.SOURCES:
        cmd = [b._hipcc(), f"--offload-arch={b.ARCH}", *b.FLAGS, f"-I{b.INCLUDE}", f"-I{b.CSRC}", "-S", "--cuda-device-only",
               os.path.join(b.CSRC, src), "-o", os.path.join(outdir, src.replace(".hip", ".s"))]
        procs.append((src, subprocess.Popen(cmd, stderr=subprocess.DEVNULL)))
    for src, p in procs:
        if p.wait() != 0:
            sys.exit(f"hipcc failed on {src}")


def kernels(path):
    """{mangled name: (normalised instruction text, descriptor figures)} of one assembly file."""
    text = open(path).read()
    desc = {}
    for m in re.finditer(r"\.amdhsa_kernel (\S+)\n(.*?)\.end_amdhsa_kernel", text, re.S):
        desc[m.group(1)] = tuple(re.search(re.escape(k) + r"\s+(\S+)", m.group(2)).group(1) for k in DESC)
    out = {}
    for name in desc:
        m = re.search(r"^" + re.escape(name) + r":[^\n]*\n(.*?)^\.Lfunc_end\d+:", text, re.S | re.M)
        body = []
        for line in m.group(1).split("\n"):
            line = line.split(";")[0].rstrip()
            if line:
                body.append(line)
        body = "\n".join(body).replace(name[2:], "KERNEL")        # the kernel itself and its function-local LDS symbols
        out[name] = (re.sub(r"\.LBB\d+_", ".LBB_", body), desc[name])
    return out


def pool(sdir):
    """{mangled name: [(unit, body, descriptor figures), ...]} over every .s file of one tree."""
    out = {}
    for unit in sorted(f for f in os.listdir(sdir) if f.endswith(".s")):
        for name, (body, desc) in kernels(os.path.join(sdir, unit)).items():
            out.setdefault(name, []).append((unit, body, desc))
    return out


def compare(pdir, ndir, renames):
    par, new = pool(pdir), pool(ndir)
    bad = 0
    used, same, moved = set(), 0, 0
    per_unit = {}                                # new unit -> [kernels, identical]
    for name, found in sorted(new.items(), key=lambda kv: (kv[1][0][0], kv[0])):
        unit, body, desc = found[0]
        cnt = per_unit.setdefault(unit, [0, 0])
        cnt[0] += 1
        if len(found) > 1:                       # one kernel, one unit: a second copy is dead weight in the library
            print(f"DUPLICATED in {', '.join(u for u, _, _ in found)}: {name}")
            bad += 1
        pname = name if name in par else next((p for sub, p in renames if sub in name), None)
        if pname not in par:
            print(f"{unit}: NO PARENT for {name}")
            bad += 1
            continue
        used.add(pname)
        punit, pbody, pdesc = par[pname][0]
        if pname != name:
            print(f"{unit}: {name}\n    compared with parent {pname}")
        if (body, desc) == (pbody, pdesc):
            same += 1
            cnt[1] += 1
            moved += punit != unit
        else:
            what = "descriptor " + " ".join(f"{a}->{b}" for a, b in zip(pdesc, desc)) if desc != pdesc else "instructions"
            # class B: the same instructions in the same places, only operands differ (register numbers, operand order)
            mnem = [[line.split()[0] for line in b.split("\n")] for b in (pbody, body)]
            cls = "class B" if desc == pdesc and mnem[0] == mnem[1] else "not class B"
            print(f"{unit}: DIFFERS ({what}; {cls}): {name}" + (f" (parent: {punit})" if punit != unit else ""))
            bad += 1
    gone = [p for p in par if p not in used]
    for p in gone:
        print(f"{par[p][0][0]}: removed {p}")
    for unit, (n, s) in sorted(per_unit.items()):
        print(f"{unit}: {n} kernels compared, {s} identical")
    print(f"total: {len(new)} compared, {same} identical ({moved} of them in another unit), {len(gone)} removed, {bad} defects")
    return 1 if bad else 0


if __name__ == "__main__":
    a = sys.argv[1:]
    if len(a) >= 3 and a[0] == "emit":
        emit(os.path.abspath(a[1]), a[2], a[3:])
    elif len(a) >= 3 and a[0] == "compare":
        sys.exit(compare(a[1], a[2], [tuple(r.split("=", 1)) for r in a[3:]]))
    else:
        sys.exit(__doc__)
