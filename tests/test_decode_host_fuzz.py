"""Sanitized stand-alone fuzz of the host build of the ingest decoders.

tests/native/decode_fuzz.cpp (its own main) is compiled with
`g++ -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all` against
ops/csrc/l7_decode.h / l4_decode.h -- the text the GPU kernels compile --
and dfcpu.cpp's span generator, and run as a child process. Nothing is
loaded into Python. It decodes 256 generated spans and 256 generated flows,
each under: truncation at every length, and MUTATIONS times each of a bit
flip, a byte overwritten with 0xFF and a length byte overwritten with
0x80..0xFF, every mutated record alone in a fresh heap buffer of its length
rounded up to 8. AddressSanitizer is the bounds oracle, the program's end
the hang oracle, and it checks every emitted string ref against [0, len).

MUTATIONS = 256 per record and kind: 549,662 decodes; measured 5.2 s for
compile plus run (about 3.5 s of it the compile), far under the 20 s bound,
which leaves room on a slower machine.
"""
import shutil
import subprocess
from pathlib import Path

import pytest

from deepflow_amd.gen.flows import FlowGenConfig, gen_flow_payload

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "deepflow_amd" / "ops" / "csrc"
MUTATIONS = 256


def test_decode_host_fuzz(tmp_path):
    if shutil.which("g++") is None:
        pytest.fail("g++ is required to build the fuzz program")
    exe = tmp_path / "decode_fuzz"
    cc = subprocess.run(
        ["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined",
         "-fno-sanitize-recover=all", f"-I{CSRC}",
         str(ROOT / "tests" / "native" / "decode_fuzz.cpp"),
         str(CSRC / "dfcpu.cpp"), "-ldl", "-o", str(exe)],
        capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr[-4000:]
    flows = tmp_path / "flows.bin"
    flows.write_bytes(gen_flow_payload(FlowGenConfig(
        n=256, seed=5, acl_rate_pct=50, ip6_rate_pct=30)))
    run = subprocess.run([str(exe), str(flows), str(MUTATIONS)],
                         capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, (run.stdout + run.stderr)[-4000:]
    print(run.stdout)
    assert "ok" in run.stdout
