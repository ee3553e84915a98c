"""Build tests/devunit/_devunit.so (hipcc, gfx950).  Test infrastructure, see devunit.hip.

The compiler flags are the product's: CXXFLAGS and ARCH are read from pydeseq2_amd/csrc/Makefile, not restated, so
that the device math is tested under the same -ffp-contract and -O level the kernels are built with."""
import os
import re
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
SRC = os.path.join(HERE, "devunit.hip")  # dsq_math.h, dsq_wave.h
SRC_LINALG = os.path.join(HERE, "devunit_linalg.hip")  # dsq_wide.h, dsq_wider.h, row_chol_solve
SRC_STATS = os.path.join(HERE, "devunit_stats.hip")  # dsq_stats.h, dsq_lds_sort.h
SRC_OPTIM = os.path.join(HERE, "devunit_optim.hip")  # dsq_lbfgsb_wave.h, dsq_lbfgsb.h, dsq_lbfgsb_par.h
SRC_ALPHA = os.path.join(HERE, "devunit_alpha.hip")  # dsq_alpha.h; launches the two row-kernel units below
SRC_TREND = os.path.join(HERE, "devunit_trend.hip")  # dsq_trend_grid.h; launches the trend unit below
SRC_SHRINK = os.path.join(HERE, "devunit_shrink.hip")  # dsq_shrink.h: shrink_fn, shrink_fn_wide
INC = os.path.join(ROOT, "pydeseq2_amd", "csrc")
# the product's row kernels of the dispersion fit, unchanged and with the product's flags: devunit_alpha.hip calls their
# launch_* entry points (dsq_launch.h)
SRC_ROWS = os.path.join(INC, "dsq_k_alpha_rows.hip")
SRC_ROWSC = os.path.join(INC, "dsq_k_alpha_rowsc.hip")
# the product's trend kernels and their launchers, likewise: devunit_trend.hip calls launch_trend_fit / _glm / _loss_grad
SRC_KTREND = os.path.join(INC, "dsq_k_trend.hip")
SRCS = [SRC, SRC_LINALG, SRC_STATS, SRC_OPTIM, SRC_ALPHA, SRC_TREND, SRC_SHRINK, SRC_ROWS, SRC_ROWSC, SRC_KTREND]
HOST_H = os.path.join(HERE, "devunit_host.h")
OUT = os.path.join(HERE, "_devunit.so")
MAKEFILE = os.path.join(INC, "Makefile")
HIPCC = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")


def makefile_var(name):
    """A variable of the Makefile's simple `NAME = value` / `NAME ?= value` assignments, $(NAME) references expanded."""
    raw = {}
    with open(MAKEFILE) as f:
        for line in f:
            m = re.match(r"^([A-Za-z_][A-Za-z0-9_]*)\s*\??=\s*(.*?)\s*$", line)
            if m and m.group(1) not in raw:
                raw[m.group(1)] = m.group(2)

    def expand(v, depth=0):
        if depth > 8:
            raise RuntimeError(f"{MAKEFILE}: recursive variable in {v!r}")
        return re.sub(r"\$\((\w+)\)", lambda m: expand(raw[m.group(1)], depth + 1), v)

    return expand(raw[name])


def cxxflags():
    """The product's CXXFLAGS as a list (ARCH expanded)."""
    return makefile_var("CXXFLAGS").split()


def compile_cmd(out=OUT):
    return [HIPCC, *cxxflags(), "-shared", "-I", INC, *SRCS, "-o", out]


def asm_cmd(out):
    """Device assembly of the library: shows which branches of the headers the device build took.  One output file
    takes one input, so the other units are read in front of the first (-include); their names do not collide."""
    return [HIPCC, *cxxflags(), "--cuda-device-only", "-S", "-I", INC, "--include=" + SRC_LINALG, "--include=" + SRC_STATS,
            "--include=" + SRC_OPTIM, "--include=" + SRC_ALPHA, "--include=" + SRC_SHRINK, SRC, "-o", out]


def build(force=False):
    deps = [*SRCS, HOST_H, MAKEFILE] + [os.path.join(INC, f) for f in os.listdir(INC) if f.endswith(".h")]
    deps.append(os.path.join(ROOT, "include", "deseq_hip.h"))
    if not force and os.path.exists(OUT) and all(
        os.path.getmtime(OUT) >= os.path.getmtime(d) for d in deps
    ):
        return OUT
    tmp = os.path.join(HERE, f"_devunit.{os.getpid()}.so")  # atomic replace: a concurrent loader never sees half a file
    subprocess.run(compile_cmd(tmp), check=True)
    os.replace(tmp, OUT)
    return OUT


if __name__ == "__main__":
    print(build(force=True))
