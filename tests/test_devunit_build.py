"""CPU-side checks of tests/devunit (no GPU needed: hipcc cross-compiles for gfx950).

* the library builds, with exactly the CXXFLAGS that csrc/Makefile gives the product (asked of make itself);
* its device assembly contains the device-only instructions (v_rcp_f64 / v_rsq_f64, the permlane swaps, DPP row_ror and
  row_half_mirror, the fp64 MFMA),
  so the tests in test_devunit_*.py run the device branches of the headers, not the host ones;
* the four table headers, parsed from the source, are the correctly rounded values entry by entry (mpmath, 120 bits),
  independently of the tools/gen_* scripts that wrote them."""
import importlib
import os
import re
import shutil
import subprocess

import mpmath
import numpy as np
import pytest

dub = importlib.import_module("tests.devunit.build")  # (the package exports the function build())

CSRC = dub.INC
needs_hipcc = pytest.mark.skipif(not os.path.exists(dub.HIPCC), reason="hipcc not installed")


def make_cxxflags():
    """CXXFLAGS as make expands it"""
    out = subprocess.run(["make", "-s", "-C", CSRC, "--no-print-directory", "--eval",
                          "devunit-print-cxxflags: ; @echo $(CXXFLAGS)", "devunit-print-cxxflags"],
                         check=True, capture_output=True, text=True).stdout
    return out.split()


@pytest.mark.skipif(shutil.which("make") is None, reason="make not installed")
def test_flags_are_the_makefiles():
    flags = make_cxxflags()
    assert "-ffp-contract=fast" in flags and "--offload-arch=gfx950" in flags
    cmd = dub.compile_cmd()
    assert cmd[1:1 + len(flags)] == flags
    assert not any(c.startswith("-ffp-contract") for c in cmd[1 + len(flags):])
    assert dub.asm_cmd("x.s")[1:1 + len(flags)] == flags


def test_sources_are_the_test_units_and_the_product_units_they_launch():
    """devunit_alpha.hip launches the product's row kernels and devunit_trend.hip the product's trend kernels: those
    three units are compiled into the library from csrc/ itself, with the same flags, and stay out of the assembly
    listing (which shows the branches the HEADERS took)."""
    rel = [os.path.relpath(p, dub.ROOT) for p in dub.SRCS]
    assert rel == ["tests/devunit/devunit.hip", "tests/devunit/devunit_linalg.hip", "tests/devunit/devunit_stats.hip",
                   "tests/devunit/devunit_optim.hip", "tests/devunit/devunit_alpha.hip", "tests/devunit/devunit_trend.hip",
                   "tests/devunit/devunit_shrink.hip", "pydeseq2_amd/csrc/dsq_k_alpha_rows.hip", "pydeseq2_amd/csrc/dsq_k_alpha_rowsc.hip",
                   "pydeseq2_amd/csrc/dsq_k_trend.hip"]
    assert all(os.path.exists(p) for p in dub.SRCS)
    cmd, asm = dub.compile_cmd(), dub.asm_cmd("x.s")
    assert all(p in cmd for p in dub.SRCS)
    assert "--include=" + dub.SRC_ALPHA in asm and "--include=" + dub.SRC_SHRINK in asm
    assert not any("dsq_k_alpha_rows" in c or "dsq_k_trend" in c for c in asm)
    # the product builds the trend unit too (a unit of its own, so that it links here without the rest of dsq_k_stats.hip)
    assert "dsq_k_trend.hip" in dub.makefile_var("SRCS").split()


@needs_hipcc
def test_builds():
    out = dub.build()
    assert os.path.getsize(out) > 0


@needs_hipcc
@pytest.mark.skipif(shutil.which("nm") is None, reason="nm not installed")
def test_the_library_has_no_undefined_product_symbol():
    """Every dsq:: function the test units call is defined by a product unit in the library: a launcher that moved to a
    unit which is not linked here would only fail when the library is loaded on the GPU machine."""
    out = dub.build()
    syms = subprocess.run(["nm", "-C", "-D", "--undefined-only", out], check=True, capture_output=True, text=True).stdout
    assert "hipLaunchKernel" in syms  # the listing is the library's
    assert [ln for ln in syms.splitlines() if "dsq::" in ln] == []
    defined = subprocess.run(["nm", "-C", "-D", "--defined-only", out], check=True, capture_output=True, text=True).stdout
    for name in ("dsq::launch_trend_fit(", "dsq::launch_trend_glm(", "dsq::launch_trend_loss_grad(",
                 "dsq::trend_grid_mem_bytes("):
        assert name in defined, name


@needs_hipcc
def test_device_assembly_takes_the_device_branches(tmp_path):
    s = tmp_path / "devunit.s"
    subprocess.run(dub.asm_cmd(str(s)), check=True, capture_output=True)
    asm = s.read_text()
    for ins in ("v_rcp_f64", "v_rsq_f64", "v_permlane32_swap", "v_permlane16_swap", "row_ror:8", "row_ror:4",
                "row_half_mirror", "row_newbcast", "ds_add_f64", "ds_read_b128", "v_mfma_f64_16x16x4"):
        assert ins in asm, ins


# ------------------------------------------------------------------------------------------------ table headers
def parse_table(header, name):
    """the initialiser list of `name` in a csrc table header (decimal or hex-float literals)"""
    src = open(os.path.join(CSRC, header)).read()
    m = re.search(r"\b" + name + r"\[(\d+)\]\s*=\s*\{", src)
    assert m, name
    body = src[m.end():src.index("};", m.end())]
    body = body.split("{")[-1]  # the device and the host declaration share one initialiser (#if / #else / #endif)
    body = "\n".join(ln for ln in body.splitlines() if not ln.lstrip().startswith(("#", "//")))
    vals = [v.strip() for v in body.replace("\n", " ").split(",") if v.strip()]
    out = np.array([float.fromhex(v) if "0x" in v else float(v) for v in vals])
    assert out.size == int(m.group(1)), (name, out.size)
    return out


def parse_const(header, name):
    src = open(os.path.join(CSRC, header)).read()
    m = re.search(r"\b" + name + r"\s*=\s*([0-9a-fA-Fx.p+-]+)", src)
    v = m.group(1)
    return float.fromhex(v) if "0x" in v else float(v)


def cr(v):
    return float(mpmath.mpf(v))


def same_bits(a, b):
    return np.asarray(a, np.float64).view(np.int64).tolist() == np.asarray(b, np.float64).view(np.int64).tolist()


def test_lgamma_int_table():
    with mpmath.workprec(120):
        ref = [cr(mpmath.loggamma(k + 1)) for k in range(256)]
    assert same_bits(parse_table("dsq_lgamma_int.h", "kLgammaInt"), ref)


def test_log_int_table():
    with mpmath.workprec(120):
        ref = [0.0] + [cr(mpmath.log(k)) for k in range(1, 256)]  # entry 0 unused
    assert same_bits(parse_table("dsq_lgamma_int.h", "kLogInt"), ref)


def test_log_table():
    # {rc_j = double(1 / c_j), T_j = -log(rc_j)} with c_j = 1 + j/128, both correctly rounded (T of the ROUNDED rc)
    t = parse_table("dsq_log_table.h", "kLogTab")
    with mpmath.workprec(120):
        rc = [cr(mpmath.mpf(128) / (128 + j)) for j in range(128)]
        T = [cr(-mpmath.log(mpmath.mpf(r))) for r in rc]
    assert same_bits(t[0::2], rc) and same_bits(t[1::2], T)


def test_exp_table_and_constants():
    t = parse_table("dsq_exp_table.h", "kExpTab")
    with mpmath.workprec(120):
        assert same_bits(t, [cr(mpmath.mpf(2) ** (mpmath.mpf(j) / 128)) for j in range(128)])
        step = mpmath.log(2) / 128
        assert parse_const("dsq_exp_table.h", "kExpInvStep") == cr(1 / step)
        hi, lo = parse_const("dsq_exp_table.h", "kExpStepHi"), parse_const("dsq_exp_table.h", "kExpStepLo")
        # hi has trailing zero bits so that k * hi is exact for every |k| the reduction meets (< 2^18), and
        # lo is the correctly rounded remainder
        m, _ = np.frexp(hi)
        assert (int(m * 2.0**53) & ((1 << 18) - 1)) == 0
        assert lo == cr(step - mpmath.mpf(hi))
