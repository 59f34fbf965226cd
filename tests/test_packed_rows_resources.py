"""CPU (compile only): every kept instantiation of the packed pass (csrc/gemv_packed.hpp, rows per burst R) reports no
scratch, and the 1024-thread ones at most 128 VGPRs - one workgroup of 16 waves per CU is 4 waves per SIMD, and a kernel
over 128 registers could not be launched at that size.  Read from the compiler's resource remarks alone."""
import re

import pytest


@pytest.mark.timeout(600)
def test_packed_pass_instantiations_fit(tmp_path):
    from fastoptsolver_amd import build
    err = build.compile_unit("fos_plan", extra=["-Rpass-analysis=kernel-resource-usage"], out=str(tmp_path / "fos_plan.o"),
                             verbose=False).stderr
    kernels, cur = {}, None
    for line in err.splitlines():
        m = re.search(r"remark:\s+Function Name:\s+(\S+)", line)
        if m:
            cur = m.group(1)
            kernels[cur] = {}
            continue
        m = re.search(r"remark:\s+(VGPRs Spill|ScratchSize \[bytes/lane\]|VGPRs):\s+(\d+)", line)
        if m and cur:
            kernels[cur][m.group(1)] = int(m.group(2))
    # _ZN3fos2pk18gemv_packed_kernelILi<THREADS>ELb<IL>ELi<R>ELb<ADJ>EE...
    seen = {}
    for name, res in kernels.items():
        m = re.match(r"_ZN3fos2pk18gemv_packed_kernelILi(\d+)ELb([01])ELi(\d+)ELb([01])EE", name)
        if m:
            seen[(int(m.group(1)), int(m.group(2)), int(m.group(3)), int(m.group(4)))] = res
    want = {(1024, il, r, 0) for il in (0, 1) for r in (1, 2, 3)} | {(512, il, r, 0) for il in (0, 1) for r in (1, 2, 3, 4)}
    assert set(seen) == want, sorted(set(seen) ^ want)
    for inst, res in sorted(seen.items()):
        assert res.get("ScratchSize [bytes/lane]", -1) == 0 and res.get("VGPRs Spill", 0) == 0, (inst, res)
        if inst[0] == 1024:
            assert 0 < res["VGPRs"] <= 128, (inst, res)
