"""Build tests/hostvoom/_hostvoom.so (g++, host only).  Test infrastructure, see hostvoom.cpp."""
import glob
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
SRC = os.path.join(HERE, "hostvoom.cpp")
OUT = os.path.join(HERE, "_hostvoom.so")
INC = os.path.join(ROOT, "pydeseq2_amd", "csrc")


def build(force=False):
    deps = [SRC] + glob.glob(os.path.join(INC, "*.h"))  # dsq_voom.h sits on dsq_wide.h and most of what that includes
    if not force and os.path.exists(OUT) and all(
        os.path.getmtime(OUT) >= os.path.getmtime(d) for d in deps
    ):
        return OUT
    cmd = ["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-ffp-contract=off", "-I", INC, SRC,
           "-o", OUT]
    subprocess.run(cmd, check=True)
    return OUT


if __name__ == "__main__":
    print(build(force=True))
