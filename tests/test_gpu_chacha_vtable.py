"""The ChaCha20-Poly1305 picotls objects through picotls' own core, side by side with ptls_openssl_chacha20poly1305 /
ptls_openssl_chacha20 (tests/c/test_chacha_vtable.c)."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu


def test_chacha_vtable_pairs():
    exe = os.path.join(os.path.dirname(os.path.abspath(__file__)), "c", "_bin", "test_chacha_vtable")
    if not os.path.exists(exe):
        pytest.skip("tests/c/_bin/test_chacha_vtable not built (needs picotls headers at build time)")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert "not ok" not in r.stdout and "# 0 failed" in r.stdout
