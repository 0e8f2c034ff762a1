"""A reduction batch is published to the host by k_publish (open_pcc_metric_amd/csrc/pccm_point.hip), one wave behind the
batch's last kernel: a system-scope release (buffer_wbl2), then the bump of the context's completion counter in host memory.
The write-back must be complete before the counter moves, or the host may read numbers still on their way; hipcc is known to
drop the s_waitcnt vmcnt(0) behind buffer_wbl2 in some shapes of code, which is why an inline-asm wait sits there too.  This
test compiles the file to gfx950 ISA (hipcc cross-compiles without a GPU) and checks the kernel."""
import os
import re
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "open_pcc_metric_amd", "csrc", "pccm_point.hip")


def kernel_body(asm, name):
    body, inside = [], False
    for ln in asm.split("\n"):
        if re.match(rf"^{name}:", ln):
            inside = True
        elif inside and ln.startswith(".Lfunc_end"):
            return body
        elif inside:
            body.append(ln.strip())
    return None


def test_counter_update_waits_for_the_write_back():
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "point.s")
        subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-I" + os.path.join(ROOT, "include"),
                        "-S", "--cuda-device-only", "-o", out, SRC], check=True, stderr=subprocess.DEVNULL, timeout=900)
        body = kernel_body(open(out).read(), r"_ZN4pccm9k_publishEPy")
    assert body, "k_publish not found in the ISA"
    wb = [i for i, ln in enumerate(body) if ln.startswith("buffer_wbl2")]
    assert len(wb) == 1 and "sc0 sc1" in body[wb[0]], body          # one release, at system scope
    ctr = [i for i, ln in enumerate(body) if ln.startswith("global_atomic_add_x2")]
    assert len(ctr) == 1 and ctr[0] > wb[0], "no 64-bit counter update behind the release"
    between = body[wb[0] + 1:ctr[0]]
    assert "s_waitcnt vmcnt(0)" in between, "the counter update does not wait for the write-back:\n" + "\n".join(between)
    # nothing else of the kernel touches memory: the counter is the only store
    mem = [ln for ln in body if re.match(r"(global|buffer|flat|scratch)_", ln)]
    assert mem == [body[wb[0]], body[ctr[0]]], mem
