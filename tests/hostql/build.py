"""Build tests/hostql/_hostql.so (g++, host only).  Test infrastructure, see hostql.cpp."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
SRC = os.path.join(HERE, "hostql.cpp")
OUT = os.path.join(HERE, "_hostql.so")
INC = os.path.join(ROOT, "pydeseq2_amd", "csrc")


def build(force=False):
    deps = [SRC] + [os.path.join(INC, f) for f in ("dsq_ql.h", "dsq_lrt.h", "dsq_wave.h", "dsq_math.h",
                                                    "dsq_exp_table.h", "dsq_log_table.h")]
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
