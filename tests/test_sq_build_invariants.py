"""The exact rescoring kernels over the fp16 codes (row source ROWS_F16T) and the threshold kernel instantiated for them compile without
scratch; the fused filter over the codes spills only where its fp32 twin does (checked on the ISA hipcc emits, CPU only)."""
import os, re, shutil, subprocess, tempfile
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "..", "lightretriever_amd", "csrc", "lrx_search.hip")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


@pytest.fixture(scope="module")
def search_isa():
    if not (os.path.exists(HIPCC) or shutil.which(HIPCC)):
        pytest.skip("no hipcc")
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "s.s")
        subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", "-o", out, SRC], check=True,
                       stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        return open(out).read()


def bodies(isa, prefix):
    found = re.findall(r"^(%s\w*):[^\n]*\n(.*?)s_endpgm" % prefix, isa, re.S | re.M)
    assert found, prefix
    return found


@pytest.mark.parametrize("kernel", ["_Z13k_refine_bandILi1E", "_Z20k_rescore_row_groupsILi1E", "_Z13k_refine_topkILi1E",
                                    "_Z21k_topk_select_rescoreILi1E", "_Z18k_sample_thresholdILi1E"])
def test_codes_rescoring_kernels_have_no_scratch(search_isa, kernel):
    for name, body in bodies(search_isa, kernel):
        assert "scratch_" not in body, name


def test_fused_filter_over_codes_spills_only_where_its_fp32_twin_does(search_isa):
    # (k_filter_fused at 7 and 8 query tiles spills in both instantiations; the error bound over the codes adds no spill of its own)
    fused = dict(bodies(search_isa, "_Z14k_filter_fusedILi"))
    codes = {n: b for n, b in fused.items() if re.match(r"_Z14k_filter_fusedILi\d+ELi\d+ELi\d+ELi1EEv", n)}
    assert len(codes) == 16
    for name, body in codes.items():
        twin = name.replace("ELi1EEv", "ELi0EEv", 1)
        assert ("scratch_" in body) == ("scratch_" in fused[twin]), name
