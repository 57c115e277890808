"""client::ResponseSession of the C++ host mirror (include/amphora.hpp) run as
a program (tests/cpp/client_session_test.cpp): KAT-3's structure and a
three-party round trip handed in party by party, in three orders, against
host-computed values and the whole-call mirrors on the same texts."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


@pytest.mark.gpu
def test_cpp_response_session():
    import build_native
    r = subprocess.run([build_native.build_client_session_test()], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "client session mirror ok" in r.stdout, r.stdout + r.stderr
