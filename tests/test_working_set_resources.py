"""CPU (compile only): the kernels of csrc/working_set.hpp neither spill nor use scratch, and hold the LDS their header states.
Modelled on tests/test_no_spills.py, which compiles the whole library (these kernels included, through fos_fista.hip); this file
compiles the header alone with the library's flags, so that it takes seconds and names the two kernels."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

UNIT = """
#include "working_set.hpp"
// every instantiation fos_gather_columns / fos_kkt_scan launch
void* fos_working_set_kernels[] = {(void*)fos::gather_columns_kernel<2>, (void*)fos::gather_columns_kernel<4>, (void*)fos::kkt_scan_kernel};
"""


def test_working_set_kernels_do_not_spill(tmp_path):
    from fastoptsolver_amd import build
    src = tmp_path / "ws_unit.hip"
    src.write_text(UNIT)
    cmd = [build.hipcc_path(), *build.FLAGS, "-I", build.CSRC, "-Rpass-analysis=kernel-resource-usage", "-c", "-o", str(tmp_path / "ws_unit.o"),
           str(src)]
    out = subprocess.run(cmd, check=True, capture_output=True, text=True).stderr
    kernels, cur = {}, None
    for line in out.splitlines():
        m = re.search(r"remark:\s+Function Name:\s+(\S+)", line)
        if m:
            cur = m.group(1)
            kernels[cur] = {}
            continue
        m = re.search(r"remark:\s+(VGPRs Spill|SGPRs Spill|ScratchSize \[bytes/lane\]|VGPRs|LDS Size \[bytes/block\]):\s+(\d+)", line)
        if m and cur:
            kernels[cur][m.group(1)] = int(m.group(2))
    gather = {k: v for k, v in kernels.items() if "gather_columns_kernel" in k}
    scan = {k: v for k, v in kernels.items() if "kkt_scan_kernel" in k}
    assert len(gather) == 2 and len(scan) == 1, sorted(kernels)
    for k, v in {**gather, **scan}.items():
        assert not v.get("VGPRs Spill", 0) and not v.get("SGPRs Spill", 0) and not v.get("ScratchSize [bytes/lane]", 0), (k, v)
        assert v["VGPRs"] <= 64, (k, v)                           # eight waves per SIMD: the gather hides latency by occupancy
    assert all(v["LDS Size [bytes/block]"] == 32768 for v in gather.values())      # WS_IDX_CHUNK int32 indices
    assert all(v["LDS Size [bytes/block]"] == 64 for v in scan.values())           # the 16 wave counts
    # the instantiations above are the ones the library launches
    with open(os.path.join(build.CSRC, "fos_fista.hip")) as fh:
        text = fh.read()
    assert set(re.findall(r"fos::gather_columns_kernel<(\d)>", text)) == {"2", "4"} and "fos::kkt_scan_kernel" in text
