"""CPU (compile only): the twelve instantiations of csrc/pointwise_link.hpp neither spill nor use scratch.  Modelled on
tests/test_working_set_resources.py: the header alone is compiled with the library's flags, so that it takes seconds."""
import re
import subprocess

LINKS, FOLDS = ("LINK_HUBER", "LINK_SQUARED_HINGE"), ("FOLD_OFF", "FOLD_TRAIN", "FOLD_HELD")
UNIT = '#include "pointwise_link.hpp"\n// every instantiation launch_pointwise_link launches\nvoid* fos_pointwise_link_kernels[] = {\n' + \
    "".join(f"  (void*)fos::pointwise_link_kernel<fos::{k}, fos::{f}, {w}>,\n" for k in LINKS for f in FOLDS for w in ("false", "true")) + "};\n"


def test_pointwise_link_kernels_do_not_spill(tmp_path):
    from fastoptsolver_amd import build
    src = tmp_path / "link_unit.hip"
    src.write_text(UNIT)
    cmd = [build.hipcc_path(), *build.FLAGS, "-I", build.CSRC, "-Rpass-analysis=kernel-resource-usage", "-c", "-o", str(tmp_path / "link_unit.o"),
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
    link = {k: v for k, v in kernels.items() if "pointwise_link_kernel" in k}
    assert len(link) == 12, sorted(kernels)
    for k, v in link.items():
        print(k, v)
        assert not v.get("VGPRs Spill", 0) and not v.get("SGPRs Spill", 0) and not v.get("ScratchSize [bytes/lane]", 0), (k, v)
        assert v["VGPRs"] <= 64, (k, v)                           # eight waves per SIMD: the link hides latency by occupancy
        assert v["LDS Size [bytes/block]"] == 16 * 16 * 8, (k, v)  # one fp64 per (16-lane row of the workgroup, column)
