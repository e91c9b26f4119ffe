"""ORACLE — TEST INFRASTRUCTURE ONLY.  The recipe that compiles the reference's own Correlation / Resample2d / ChannelNorm
kernels for the CPU, into oracle/_ref/ (never committed):

  1. read the three .cu files from the reference checkout (absent -> nothing is built, build() returns None);
  2. rewrite every `k<<<grid, block, shmem, stream>>>` into `coc::launch(k, grid, block, shmem, stream)` — the ONLY change to
     their text; `<THC.h>`, `<THCGeneral.h>` and "correlation_cuda_kernel.h" resolve to the stand-ins next to this file through
     the include path.  The number of rewritten launches must be 7 / 3 / 2 and no `<<<` may remain, else the build fails;
  3. g++ -O2 -ffp-contract=off (the convention of oracle/Makefile) -> oracle/_ref/libflowtrack_ref_ops.so; where the build CPU
     has FMA, a second library with -ffp-contract=fast -mfma -> libflowtrack_ref_ops_fma.so, used only to bound what nvcc's
     default contraction could change.
"""
from __future__ import annotations

import os
import re
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(os.path.dirname(HERE), "_ref")
LIB = os.path.join(OUT, "libflowtrack_ref_ops.so")
LIB_FMA = os.path.join(OUT, "libflowtrack_ref_ops_fma.so")
REF = os.environ.get("FLOWTRACK_REFERENCE", "/root/reference")      # where tests/golden/make_golden.py finds it too

# file below <reference>/lib/flownet/networks, launches it must contain
SOURCES = (
    ("correlation_package/src/correlation_cuda_kernel.cu", 7),
    ("resample2d_package/src/Resample2d_kernel.cu", 3),
    ("channelnorm_package/src/ChannelNorm_kernel.cu", 2),
)
LAUNCH_COUNTS = {os.path.basename(p): n for p, n in SOURCES}
_LAUNCH = re.compile(r"(\w+)\s*<\s*<\s*<(.*?)>\s*>\s*>", re.S)
_LEFTOVER = re.compile(r"<\s*<\s*<|>\s*>\s*>")


def _split_top_level(text):
    parts, depth, cur = [], 0, ""
    for ch in text:
        if ch == "," and depth == 0:
            parts.append(cur.strip())
            cur = ""
            continue
        depth += ch in "([{"
        depth -= ch in ")]}"
        cur += ch
    parts.append(cur.strip())
    return parts


def rewrite_launches(text, want, name="<text>"):
    """(rewritten text, count).  Raises when the count is not `want` or a chevron is left."""
    count = 0

    def sub(m):
        nonlocal count
        cfg = _split_top_level(m.group(2))
        if len(cfg) != 4:
            raise RuntimeError(f"{name}: launch of {m.group(1)} has {len(cfg)} configuration arguments, expected 4")
        count += 1
        return f"coc::launch({m.group(1)}, {', '.join(cfg)})"

    out = _LAUNCH.sub(sub, text)
    if count != want:
        raise RuntimeError(f"{name}: rewrote {count} kernel launches, expected {want}")
    if _LEFTOVER.search(out):
        raise RuntimeError(f"{name}: a launch chevron is left after the rewrite")
    return out, count


def source_paths():
    return [os.path.join(REF, "lib", "flownet", "networks", rel) for rel, _ in SOURCES]


def reference_present():
    return all(os.path.isfile(p) and os.access(p, os.R_OK) for p in source_paths())


def cpu_has_fma():
    try:
        with open("/proc/cpuinfo") as f:
            return any(line.startswith("flags") and " fma " in line + " " for line in f)
    except OSError:
        return False


def _stale(target, deps):
    return not os.path.exists(target) or any(os.path.getmtime(target) < os.path.getmtime(d) for d in deps)


def build(force: bool = False):
    """Returns LIB, or None where the reference is absent (a prebuilt oracle/_ref/ is then used as it is)."""
    if not reference_present():
        return LIB if os.path.exists(LIB) else None
    own = [os.path.join(HERE, f) for f in sorted(os.listdir(HERE)) if f.endswith((".h", ".py"))]
    want_fma = cpu_has_fma()
    if not force and not _stale(LIB, source_paths() + own) and not (want_fma and _stale(LIB_FMA, source_paths() + own)):
        return LIB
    os.makedirs(OUT, exist_ok=True)
    generated = []
    for path, (_, want) in zip(source_paths(), SOURCES):
        with open(path) as f:
            text, _ = rewrite_launches(f.read(), want, os.path.basename(path))
        gen = os.path.join(OUT, os.path.splitext(os.path.basename(path))[0] + ".cpp")
        with open(gen, "w") as f:
            f.write(text)
        generated.append(gen)
    cxx = os.environ.get("CXX", "g++")
    base = [cxx, "-O2", "-fPIC", "-shared", "-std=c++14", "-w", "-I", HERE]
    subprocess.check_call(base + ["-ffp-contract=off"] + generated + ["-o", LIB])
    if want_fma:
        subprocess.check_call(base + ["-ffp-contract=fast", "-mfma"] + generated + ["-o", LIB_FMA])
    return LIB


if __name__ == "__main__":
    print(build(force=True))
