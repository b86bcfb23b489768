"""The one build recipe of the SIMT emulator: tests/simt/libsimt_ffb6d.so, every kernel source of the product library
(ffb6d_amd/csrc/*.hip, read from the directory, minus EXCLUDED) compiled for the HOST against the emulator (tests/simt/simt.*,
fake/hip/hip_runtime.h), and load(), which every CPU test that runs a kernel takes the library from.

    python -m tests.simt.build           # build (or bring up to date) and print the library's path

Shaped like ffb6d_amd/build.py: one object per source in tests/simt/_build, recompiled only when it is older than its source, a
header of csrc/ or include/, or a file of the emulator itself; compiles run in parallel; one link.  A new csrc/*.hip is in the
emulator without an edit here, and one that does not compile for the host fails this build instead of being silently absent.
FLAGS and INCLUDES are the emulator's code generation (-ffp-contract=off as the product build: bit-exactness rests on it); a
consumer that needs different code generation (scripts/icp_instances_sanitize.py) composes them with its own flags.

The kernel sources are used as they are, except for mechanical substitutions made on a scratch copy (transformed()):
  * the declaration of the dynamic shared array becomes a pointer to the emulator's buffer; `kernel<<<...>>>(...)` launches are
    rewritten into the hipLaunchKernelGGL macro (which the fake runtime maps to the emulator);
  * where a wave reads LDS data that OTHER lanes of the same wave wrote without any instruction in between that the emulator
    treats as a rendezvous (hardware runs a wave in lock step, fibers do not), a `simt::wave_sync()` is inserted: one place,
    between the epilogue of mlp_pm_stream_kernel (lanes deposit result rows in the wave's LDS image) and the whole-row stores.
Test infrastructure only."""
import ctypes
import os
import re
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
CSRC = os.path.join(ROOT, "ffb6d_amd", "csrc")
OUT = os.path.join(HERE, "_build")
LIB = os.path.join(HERE, "libsimt_ffb6d.so")
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
FLAGS = ["-x", "c++", "-std=c++17", "-O1", "-g", "-fPIC", "-ffp-contract=off", "-Wno-unused-value", "-Wno-psabi",
         "-Wno-unknown-attributes"]
INCLUDES = ["-I" + os.path.join(HERE, "fake"), "-I" + HERE, "-I" + os.path.join(ROOT, "include"), "-I" + CSRC]

# csrc/*.hip files the emulator does not carry: file name -> reason
EXCLUDED = {"mlp_pm_split.hip": "its kernel body runs on the device only (DESIGN.md, the split-bf16 section): the fake runtime "
                                "declares no __builtin_amdgcn_sched_group_barrier"}

# statements after which a wave relies on lock-step execution for LDS traffic between its lanes
LOCKSTEP_AFTER = {"mlp_pm.hip": ["stream_epilogue<T, TM, LSM>(p, acc, img, OS, r0, l31, kh, bias_lds, HASY ? yreg : nullptr);"]}
DYN_SHARED = re.compile(r"extern\s+__shared__\s+(?:__attribute__\(\(aligned\(16\)\)\)\s+)?((?:unsigned )?\w+)\s+(\w+)\[\];")


def _split_top(text):
    parts, depth, cur = [], 0, ""
    for ch in text:
        if ch in "([{":
            depth += 1
        elif ch in ")]}":
            depth -= 1
        if ch == "," and depth == 0:
            parts.append(cur.strip())
            cur = ""
        else:
            cur += ch
    parts.append(cur.strip())
    return parts


def chevrons_to_launch_macro(src):
    """kernel<T><<<grid, block, shmem, stream>>>(args)  ->  hipLaunchKernelGGL((kernel<T>), dim3(grid), dim3(block), shmem, stream, args)"""
    out, pos = "", 0
    while True:
        i = src.find("<<<", pos)
        if i < 0:
            return out + src[pos:]
        j = src.index(">>>", i)
        k = i                                    # kernel expression: identifier [+ one template argument list] before <<<
        if src[k - 1] == ">":
            depth = 0
            while True:
                k -= 1
                depth += {">": 1, "<": -1}.get(src[k], 0)
                if depth == 0:
                    break
        while k > 0 and (src[k - 1].isalnum() or src[k - 1] in "_:"):
            k -= 1
        cfg = _split_top(src[i + 3:j]) + ["0", "0"]
        a = src.index("(", j)
        depth, e = 0, a
        while True:
            depth += {"(": 1, ")": -1}.get(src[e], 0)
            if depth == 0:
                break
            e += 1
        out += src[pos:k] + "hipLaunchKernelGGL((%s), dim3(%s), dim3(%s), %s, %s, %s)" % (
            src[k:i], cfg[0], cfg[1], cfg[2], cfg[3], src[a + 1:e])
        pos = e + 1


def transformed(name):
    os.makedirs(OUT, exist_ok=True)
    with open(os.path.join(CSRC, name)) as fh:
        src = fh.read()
    src = chevrons_to_launch_macro(src)
    src = DYN_SHARED.sub(r"\1* \2 = reinterpret_cast<\1*>(simt::dyn_shared());", src)
    for anchor in LOCKSTEP_AFTER.get(name, []):
        if src.count(anchor) != 1:
            raise RuntimeError(f"{name}: lock-step anchor not found exactly once: {anchor}")
        src = src.replace(anchor, anchor + "\n        simt::wave_sync();      // inserted by tests/simt/build.py")
    dst = os.path.join(OUT, name.replace(".hip", ".simt.cpp"))
    with open(dst, "w") as fh:
        fh.write(src)
    return dst


def sources():
    """every csrc/*.hip the emulator carries, by file name"""
    return sorted(f for f in os.listdir(CSRC) if f.endswith(".hip") and f not in EXCLUDED)


def _headers():
    """what every object depends on besides its source: the headers of csrc/ and include/, and the emulator itself"""
    deps = [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")]
    deps += [os.path.join(ROOT, "include", f) for f in os.listdir(os.path.join(ROOT, "include"))]
    deps += [os.path.join(HERE, f) for f in ("simt.cpp", "simt.h", "build.py")]
    for d, _, files in os.walk(os.path.join(HERE, "fake")):
        deps += [os.path.join(d, f) for f in files]
    return deps


def _stale(out, deps):
    if not os.path.exists(out):
        return True
    t = os.path.getmtime(out)
    return any(os.path.getmtime(d) > t for d in deps)


def _obj(name):
    return os.path.join(OUT, os.path.splitext(name)[0] + ".o")


def build():
    """One object per source (recompiled only when the source, a header or the emulator is newer), compiled in parallel, then
    linked.  Prints what it compiles.  Returns the library's path."""
    headers = _headers()
    units = [(n, os.path.join(CSRC, n)) for n in sources()] + [("simt.cpp", os.path.join(HERE, "simt.cpp"))]
    if not _stale(LIB, [src for _, src in units] + headers):
        return LIB
    from concurrent.futures import ThreadPoolExecutor
    os.makedirs(OUT, exist_ok=True)
    jobs = [(n, src) for n, src in units if _stale(_obj(n), [src] + headers)]
    jobs.sort(key=lambda j: -os.path.getsize(j[1]))          # the largest sources take longest: start them first
    if jobs:
        print("[tests.simt.build] compiling", " ".join(n for n, _ in jobs), flush=True)

    def run(job):
        name, src = job
        subprocess.run([CLANG] + FLAGS + INCLUDES + ["-c", transformed(name) if name.endswith(".hip") else src, "-o", _obj(name)],
                       check=True)

    with ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as pool:
        list(pool.map(run, jobs))
    subprocess.run([CLANG, "-shared", "-fPIC"] + [_obj(n) for n, _ in units] + ["-o", LIB + ".tmp"], check=True)
    os.replace(LIB + ".tmp", LIB)
    return LIB


_LOADED = None


def load():
    """The emulated library, built when stale, with restype / argtypes of ffb6d_amd._lib.SIGNATURES on every entry point it
    exports.  One handle per process: its switches (kernel forms, counters) are shared by everything that loads it."""
    global _LOADED
    if _LOADED is None:
        from ffb6d_amd import _lib
        lib = ctypes.CDLL(build())
        for name, (res, args) in _lib.SIGNATURES.items():
            if hasattr(lib, name):
                fn = getattr(lib, name)
                fn.restype, fn.argtypes = res, args
        _LOADED = lib
    return _LOADED


def ptr(a):
    """address of a numpy array standing in for device memory; None stays a null pointer"""
    return a.ctypes.data if a is not None else None


if __name__ == "__main__":
    print(build())
