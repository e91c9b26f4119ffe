"""Kernel-by-kernel comparison of the gfx950 device code of two trees (dev tool; needs hipcc, no GPU).

    python tools/dev/isa_diff.py emit    <tree> <outdir> [unit.hip ...]  # one .s per translation unit (default: all), the build's own flags
    python tools/dev/isa_diff.py compare <parent .s dir> <new .s dir> [new-kernel-substring=parent-mangled-name ...]

A refactor that must not change device code is checked here instead of on a GPU: every kernel (symbol with an .amdhsa_kernel block)
of the new tree has to exist in the parent under the same mangled name - or under the parent instantiation given for it on the
command line, where template parameters were dropped - with identical instruction text (comments stripped, the kernel's own name
and the function index of local labels .LBB<n>_ replaced) and equal VGPR / SGPR / AGPR-offset / LDS / scratch figures.  A kernel
that differs is reported as "class B" if it has the same number of instruction lines with the same mnemonic (first token) on every line
and equal descriptor figures, i.e. only operands changed.  Parent kernels that the new tree no longer has are listed.  Exit status 1 if
any surviving kernel differs (class B included) or has no parent."""
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


def compare(pdir, ndir, renames):
    bad = 0
    tot = [0, 0, 0]
    for unit in sorted(f for f in os.listdir(ndir) if f.endswith(".s")):
        par, new = kernels(os.path.join(pdir, unit)), kernels(os.path.join(ndir, unit))
        used, same = set(), 0
        for name, (body, desc) in new.items():
            pname = name if name in par else next((p for sub, p in renames if sub in name), None)
            if pname not in par:
                print(f"{unit}: NO PARENT for {name}")
                bad += 1
                continue
            used.add(pname)
            if pname != name:
                print(f"{unit}: {name}\n    compared with parent {pname}")
            if (body, desc) == par[pname]:
                same += 1
            else:
                what = "descriptor " + " ".join(f"{a}->{b}" for a, b in zip(par[pname][1], desc)) if desc != par[pname][1] else "instructions"
                # class B: the same instructions in the same places, only operands differ (register numbers, operand order)
                mnem = [[line.split()[0] for line in b.split("\n")] for b in (par[pname][0], body)]
                cls = "class B" if desc == par[pname][1] and mnem[0] == mnem[1] else "not class B"
                print(f"{unit}: DIFFERS ({what}; {cls}): {name}")
                bad += 1
        gone = [p for p in par if p not in used]
        for p in gone:
            print(f"{unit}: removed {p}")
        lines = [sum(1 for _ in open(os.path.join(d, unit))) for d in (pdir, ndir)]
        print(f"{unit}: {len(new)} kernels compared, {same} identical, {len(gone)} removed; assembly lines {lines[0]} -> {lines[1]}")
        for i, v in enumerate((len(new), same, len(gone))):
            tot[i] += v
    print(f"total: {tot[0]} compared, {tot[1]} identical, {tot[2]} removed, {bad} defects")
    return 1 if bad else 0


if __name__ == "__main__":
    a = sys.argv[1:]
    if len(a) >= 3 and a[0] == "emit":
        emit(os.path.abspath(a[1]), a[2], a[3:])
    elif len(a) >= 3 and a[0] == "compare":
        sys.exit(compare(a[1], a[2], [tuple(r.split("=", 1)) for r in a[3:]]))
    else:
        sys.exit(__doc__)
