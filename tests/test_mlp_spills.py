"""Register budget of the fused MLP's split kernel (no GPU needed): mlp3_split_kernel runs two waves per SIMD, so a wave owns 256 registers and the
unrolled tile body fills them.  A spilled register costs a scratch load behind an `s_waitcnt vmcnt(0)` inside the tile loop -- a wait for every
fragment load in flight.  mlp_fused.hip is compiled for the device alone with the Makefile's flags and the kernels' metadata read from the assembly:
no spill in any row-major instantiation, at most two in the column-major (XCM) ones."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# mlp3_split_kernel<Cfg<...>, SPLIT, P2S, NW, XCM, TQ>(float const*, float const*, float*, long long, unsigned*): the tail of its mangled name
SPLIT_ARGS = re.compile(r"mlp3_split_kernel.*ELi(\d+)ELi(\d+)ELi(\d+)ELb([01])ELb([01])EEEv")


def test_split_kernel_spills(tmp_path):
    out = tmp_path / "hip" / "mlp_fused.s"
    p = subprocess.run(["make", "-C", os.path.join(ROOT, "infera_amd", "csrc"), "HIP_BUILD=" + str(tmp_path), str(out)],
                       capture_output=True, text=True, timeout=1200)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-3000:]
    text = out.read_text()
    meta = text[text.index("amdhsa.kernels:"):]
    found = {False: 0, True: 0}
    for entry in meta.split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", entry).group(1)
        m = SPLIT_ARGS.search(name)
        if not m:
            continue
        xcm = m.group(4) == "1"
        spills = int(re.search(r"\.vgpr_spill_count:\s+(\d+)", entry).group(1))
        print(f"{name}: xcm={xcm} vgpr_spill_count={spills}")
        assert spills <= (2 if xcm else 0), (name, spills)
        found[xcm] += 1
    # the regression head and the three-output head, each row-major and column-major
    assert found[False] >= 2 and found[True] >= 2, found
