"""The thread protocol of a host call on the GPU platform under ThreadSanitizer, without a GPU.

pfac_amd/csrc/piece_pipeline.h holds what the threads of one PFAC_matchFromHost / PFAC_matchFromHostReduce call do together (the uploader beside the
caller's scans, the zero-fill team) with no HIP in it; tools/tsan_pipeline.cpp drives it with fake stages -- the order the stages run in for 1, 2, 3
and 7 pieces, a failure injected at every stage, the zero fill beside a consumer -- as a stand-alone program built with -fsanitize=thread.  Nothing
is loaded into python."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pfac_amd", "csrc")


def test_piece_pipeline_under_tsan():
    p = subprocess.run(["make", "-C", CSRC, "build/tsan_pipeline"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout[-3000:]
    p = subprocess.run([os.path.join(CSRC, "build", "tsan_pipeline")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert p.returncode == 0 and "ThreadSanitizer" not in p.stdout and " 0 failed" in p.stdout, p.stdout[-3000:]
