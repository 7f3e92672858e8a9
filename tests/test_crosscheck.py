"""Numerical cross-validation against the reference implementation, run as
part of the CPU suite. The reference's outputs and public names are stored
under tests/golden/ (recorded by the two scripts' --record mode), so the
checks need no reference tree."""

import os
import subprocess
import sys


def test_gradients_match_reference():
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    result = subprocess.run(
        [sys.executable, os.path.join(repo, "scripts", "crosscheck_reference.py")],
        capture_output=True, text=True, timeout=600,
    )
    assert result.returncode == 0, result.stdout[-3000:] + result.stderr[-2000:]
    assert "all within 1e-6 of the reference" in result.stdout
    assert result.stdout.count("\nOK ") + result.stdout.startswith("OK ") == 31, result.stdout[-3000:]


def test_symbol_method_ctor_parity():
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    result = subprocess.run(
        [sys.executable, os.path.join(repo, "scripts", "audit_parity.py")],
        capture_output=True, text=True, timeout=600,
    )
    assert result.returncode == 0, result.stdout[-3000:] + result.stderr[-1500:]
    assert "parity holds" in result.stdout
    assert "symbol sweep: 252 reference defs, 0 missing" in result.stdout
