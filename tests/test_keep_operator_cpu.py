"""tfqmrgpuExt_keepOperator (include/tfqmrgpu_ext.h section 9) without a GPU: the call is declared with its signature, the built library
exports it and the Python binding has it.  What it does is tests/test_gpu_keep_operator.py."""
import os
import re
import subprocess

import tfqmrgpu_amd as T
from conftest import ROOT


def test_header_declares_the_switch():
    text = open(os.path.join(ROOT, "include", "tfqmrgpu_ext.h")).read()
    assert re.search(r"tfqmrgpuStatus_t\s+tfqmrgpuExt_keepOperator\s*\(\s*tfqmrgpuBsrsvPlan_t\s+plan\s*,\s*int\s+on\s*\)\s*;", text)


def test_library_exports_the_switch():
    out = subprocess.check_output(["nm", "-D", "--defined-only", T.LIB_PATH], text=True)
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert "tfqmrgpuExt_keepOperator" in exported
    assert "tfqmrgpuExt_keepOperator" in T.EXT_SYMBOLS


def test_python_binding_has_keep_operator():
    assert callable(getattr(T.Solver, "keep_operator", None))
    assert T.lib.tfqmrgpuExt_keepOperator.argtypes is not None and len(T.lib.tfqmrgpuExt_keepOperator.argtypes) == 2
    # a pointer that is no plan is refused before anything else is looked at (host code only)
    assert T.decode(T.lib.tfqmrgpuExt_keepOperator(None, 1))[0] == 7          # TFQMRGPU_POINTER_INVALID
