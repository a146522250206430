"""The bf16 LLR instances in the BUILT library (NUMERICS.md rule 15; wr_kernels_b.hip, wr_decode_soft.hip):
  * every prefetch loop of the bf16 demod instances with the usual output set (XK = false) has its counted wait in front of
    the DMA pair, at least as many younger vector-memory instructions as that wait leaves outstanding, no other vmcnt wait
    and no scratch access -- tests/test_isa_prefetch_wait.py's rules (its name pattern also matches these instances; this
    test asserts that they are there and counts them on their own).  The XK instances pick the wait's immediate at run time;
  * the bf16 soft-decoder instances have no scratch, and each needs less LDS than the float32 instance of its class."""
import os
import re
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import test_isa_prefetch_wait as isa  # noqa: E402

LLVM = isa.LLVM


def check(tmp):
    text = isa._disassemble(tmp)
    fns = isa._functions(text)
    bf = {k: v for k, v in fns.items() if re.search(r"demod_batch_kernelILi\dELb[01]ELb0ELb1E", k)}
    assert len(bf) == 8, sorted(bf)                   # four equalisers x planes on / off
    loops = isa._prefetch_loops(bf)
    assert len(loops) >= 8 * 2 + 6 * 2, len(loops)   # BPSK / QPSK loops everywhere, 16- / 64-QAM but in COMB
    for name, eq, hb, kind, where, nst, younger, others, scratch in loops:
        assert younger >= nst, (name, where, "vmcnt(%d) with %d younger vector-memory instructions" % (nst, younger))
        assert not others and not scratch, (name, where, "a spill reload / full wait inside a prefetch loop", others, scratch)
    assert len(re.findall(r"demod_batch_kernelILi\dELb[01]ELb1ELb1E\S*>:", text)) == 8       # the any-set bf16 instances
    return len(loops)


def soft_resources(tmp):
    """{(NB, BF): (LDS bytes, scratch bytes)} of the soft-decoder instances from the code-object notes"""
    import shutil
    lib_copy, fat = os.path.join(tmp, "lib.so"), os.path.join(tmp, "fat.bin")
    shutil.copyfile(isa.LIB, lib_copy)
    subprocess.check_call(["objcopy", "--dump-section", ".hip_fatbin=" + fat, lib_copy, os.path.join(tmp, "o.so")],
                          stderr=subprocess.DEVNULL)
    data = open(fat, "rb").read()
    starts = [m.start() for m in re.finditer(b"__CLANG_OFFLOAD_BUNDLE__", data)]
    out = {}
    for n, (a, b) in enumerate(zip(starts, starts[1:] + [len(data)])):
        part, co = os.path.join(tmp, "p%d" % n), os.path.join(tmp, "c%d" % n)
        with open(part, "wb") as f:
            f.write(data[a:b])
        subprocess.check_call([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o",
                               "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--input=" + part, "--output=" + co])
        notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", co], check=True, capture_output=True,
                               text=True).stdout
        cur = {}
        for line in notes.splitlines():
            if re.match(r"^  - \.", line):
                cur = {}
            m = re.match(r"^  (?:- |  )\.(group_segment_fixed_size|private_segment_fixed_size):\s+(\d+)", line)
            if m:
                cur[m.group(1)] = int(m.group(2))
            m = re.match(r"^  (?:- |  )\.name:\s+\S*decode_soft_kernelILi(\d)ELb([01])E\S*$", line)
            if m and not line.rstrip().endswith(".kd"):
                out[(int(m.group(1)), m.group(2) == "1")] = cur
    return out


def test_bf16_soft_decoder_resources(tmp_path):
    if not os.path.exists(isa.LIB) or not os.path.exists(os.path.join(LLVM, "llvm-readelf")):
        pytest.skip("libwifirx.so or the ROCm LLVM tools are not here")
    r = soft_resources(str(tmp_path))
    for nb in (1, 2, 4, 6):
        f32, bf = r[(nb, False)], r[(nb, True)]
        assert bf["private_segment_fixed_size"] == 0, nb
        assert bf["group_segment_fixed_size"] < f32["group_segment_fixed_size"], nb
        # the rows themselves are half as large: 48 NB x 64 values of 2 bytes instead of 4
        assert f32["group_segment_fixed_size"] - bf["group_segment_fixed_size"] == 48 * nb * 64 * 2, nb


def test_bf16_prefetch_loops(tmp_path):
    """check() in a child interpreter, as tests/test_isa_prefetch_wait.py does"""
    if not os.path.exists(isa.LIB):
        pytest.skip("libwifirx.so not built")
    p = subprocess.run([sys.executable, os.path.abspath(__file__), str(tmp_path)], capture_output=True, text=True, timeout=300)
    if p.returncode == 77:
        pytest.skip(p.stdout.strip() or "tools missing")
    assert p.returncode == 0, (p.stdout[-3000:], p.stderr[-3000:])
    assert "bf16 prefetch loops checked" in p.stdout


if __name__ == "__main__":
    try:
        n = check(sys.argv[1])
    except pytest.skip.Exception as e:
        print(e)
        sys.exit(77)
    print("%d bf16 prefetch loops checked" % n)
