"""Builds scripts/icp_instances_sanitize.cpp with csrc/errors.hip + csrc/icp.hip for the HOST against the SIMT emulator (flags,
include paths and substitutions of tests/simt/build.py) under -fsanitize=address,undefined, and runs it.  An instrumented build
of its own: the emulator's cached objects carry no sanitizer.  No GPU, no Python extension involved:
    python scripts/icp_instances_sanitize.py
Exit status 0 and the program's "ok" line = no finding."""
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests.simt import build as sb      # noqa: E402

SANITIZE = ["-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]


def main():
    srcs = [sb.transformed(n) for n in ("errors.hip", "icp.hip")] + [os.path.join(sb.HERE, "simt.cpp"),
                                                                    os.path.join(ROOT, "scripts", "icp_instances_sanitize.cpp")]
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "icp_instances_sanitize")
        subprocess.run([sb.CLANG] + sb.FLAGS + SANITIZE + sb.INCLUDES + srcs + ["-o", exe], check=True)
        return subprocess.run([exe]).returncode


if __name__ == "__main__":
    sys.exit(main())
