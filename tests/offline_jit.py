"""Offline compiles of scene-specialised kernels for tests (no GPU): the embedded device headers, read
from the one list that the library itself is built from (the Makefile's DEVICE_HDR, through
`make -s print-device-hdr`), and hipcc with the JIT's own options over a source dumped with RRTE_JIT_DUMP."""
import re
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "rrte_amd" / "csrc"
HIPCC = "/opt/rocm/bin/hipcc"


def device_headers():
    """The embedded headers in include order, as paths."""
    r = subprocess.run(["make", "-s", "-C", str(CSRC), "print-device-hdr"], capture_output=True, text=True, check=True)
    return [(CSRC / h).resolve() for h in r.stdout.split()]


def stage_headers(dst: Path):
    """The headers side by side under their plain names, as hiprtc gets them (jit.hip rtc_compile): an
    include that reaches a listed header through a directory loses the directory."""
    hdrs = device_headers()
    names = "|".join(re.escape(h.name) for h in hdrs)
    for h in hdrs:
        (dst / h.name).write_text(re.sub(rf'^(#include ")[^"\n]*/((?:{names})")', r"\1\2", h.read_text(), flags=re.M))


def resources(src: Path, tmp_path: Path):
    """VGPRs / SGPRs / scratch of a dumped scene-specialised kernel: hipcc with the JIT's own options
    (jit.hip rtc_options), as tools/jit_isa.sh compiles it."""
    stage_headers(tmp_path)
    text = re.sub(r"^typedef __hip_internal.*$", "", src.read_text(), flags=re.M)
    cu = tmp_path / (src.stem + "_offline.hip")
    cu.write_text("#include <hip/hip_runtime.h>\n" + text)
    r = subprocess.run([HIPCC, "-std=c++17", "-O1", "--offload-arch=gfx950", "-ffp-contract=off",
                        "-mllvm", "-amdgpu-sched-strategy=max-ilp", "--cuda-device-only", "-S", "-o",
                        str(tmp_path / (src.stem + ".s")), "-Rpass-analysis=kernel-resource-usage", str(cu)],
                       capture_output=True, text=True, timeout=900, cwd=tmp_path)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-3000:]
    return {k: int(re.search(rf"{re.escape(k)}: (\d+)", out).group(1))
            for k in ("VGPRs", "SGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]")}

