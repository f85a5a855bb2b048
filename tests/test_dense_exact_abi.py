"""Host-side checks of the reference-order dense backend's plumbing (no GPU): the enum value in the C header and in the Python binding, and that the build compiles
piqp_amd/csrc/dense_exact.hip with floating-point contraction off -- its bitwise parity with the oracle rests on every fused operation being an explicit fma()."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_enum_value_in_the_header():
    h = open(os.path.join(ROOT, "include", "piqp_amd.h")).read()
    assert re.search(r"\bPQ_DENSE_CHOLESKY_EXACT\s*=\s*19\b", h)
    values = [int(v) for v in re.findall(r"\bPQ_(?:DENSE|SPARSE)_[A-Z_]+\s*=\s*(\d+)", h)]
    assert len(values) == len(set(values))


def test_enum_value_in_the_binding():
    import piqp_amd
    assert piqp_amd.DENSE_CHOLESKY_EXACT == 19 and piqp_amd.kkt.DENSE_CHOLESKY_EXACT == 19


def test_the_build_compiles_the_file_with_contraction_off():
    from piqp_amd import build
    assert "dense_exact.hip" in build.NO_CONTRACT
    assert os.path.join(build.SRC, "dense_exact.hip") in build.sources()
    src = open(os.path.join(build.SRC, "dense_exact.hip")).read()
    assert "mfma" not in src.lower()
