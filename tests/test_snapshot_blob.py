"""The snapshot blob's header code under AddressSanitizer and UBSan, as a stand-alone program: tests/snapshot_blob/blob_main.cpp
has its own main over the HIP-free strikeforce_amd/csrc/sf_snapshot_blob.hpp and feeds the parser valid blobs, every
truncation length and every flipped header bit, each from a heap block of exactly the blob's length.  Nothing loaded into
Python runs under a sanitizer."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_blob_parser_refuses_cleanly_under_sanitizers(tmp_path):
    exe = str(tmp_path / "blob_main")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-o", exe, os.path.join(ROOT, "tests", "snapshot_blob", "blob_main.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    m = re.search(r"^ok (\d+)$", r.stdout, re.M)
    assert m and int(m.group(1)) > 2000, r.stdout[-500:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr


def test_blob_header_is_hip_free():
    text = open(os.path.join(ROOT, "strikeforce_amd", "csrc", "sf_snapshot_blob.hpp")).read()
    includes = re.findall(r"#include\s+[<\"]([^>\"]+)[>\"]", text)
    assert includes and all(i in ("stddef.h", "stdint.h") for i in includes), includes
    assert "__device__" not in text and "__global__" not in text
