"""Builds scripts/icp_instances_sanitize.cpp with csrc/errors.hip + csrc/icp.hip for the HOST against the SIMT emulator (the
substitutions of tests/simt/build.py) under -fsanitize=address,undefined, and runs it.  No GPU, no Python extension involved:
    python scripts/icp_instances_sanitize.py
Exit status 0 and the program's "ok" line = no finding."""
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests.simt import build as sb      # noqa: E402


def main():
    os.makedirs(sb.OUT, exist_ok=True)
    srcs = [sb.transformed(n) for n in ("errors.hip", "icp.hip")] + [os.path.join(sb.HERE, "simt.cpp"),
                                                                    os.path.join(ROOT, "scripts", "icp_instances_sanitize.cpp")]
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "icp_instances_sanitize")
        cmd = [sb.CLANG, "-x", "c++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
               "-fno-sanitize-recover=undefined", "-ffp-contract=off", "-Wno-unused-value", "-Wno-psabi", "-Wno-unknown-attributes",
               "-I" + os.path.join(sb.HERE, "fake"), "-I" + sb.HERE, "-I" + os.path.join(ROOT, "include"), "-I" + sb.CSRC] + srcs + ["-o", exe]
        subprocess.run(cmd, check=True)
        return subprocess.run([exe]).returncode


if __name__ == "__main__":
    sys.exit(main())
