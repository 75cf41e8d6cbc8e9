"""The host forms that scan and then read the compiled set, under ThreadSanitizer, while another thread replaces the set.  Not a GPU test.

PFACX_matchAllFromHost, countFromHost, matchWordsFromHost (both modes), matchSpansFromHost, matchDisjointFromHost and matchLinesFromHost take their
longest pairs from hostLongestPairs and then read handle->fa; PFACX_replaceFromHost reads the pattern lengths.  Between the scan and that post-pass
nothing but the set's generation ties the pairs to the set: the post-pass holds a SetPin (pfac_amd/csrc/pfac_host.h).  A stream and a flow set are
opened, fed from the host in two pieces, flushed and closed inside one form each, so that every PFACX_...Open and ...Close (adoptNew and closeObject
of pfac_host.h) races with the thread that replaces the set too.  tools/tsan_host_forms.cpp is
a stand-alone program built with -fsanitize=thread against pfac_amd/lib/tsan/libpfac.so: four threads call every form on one host-only handle
while a fifth cycles PFACX_readPatternFromMemory through three sets -- two with the same number of patterns and other chains and lengths, one with
more.  It exits non-zero on a sanitizer report, on a call that ends in anything but the documented refusal or the single-threaded answer of ONE of
the sets, on a changed canary behind counts[], and unless every form has given every set's answer at least once.  Nothing is loaded into python."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pfac_amd", "csrc")


def test_host_forms_while_the_set_is_replaced_under_tsan():
    runtime = subprocess.run(["gcc", "-print-file-name=libtsan.so"], stdout=subprocess.PIPE, text=True).stdout.strip()
    if not os.path.isabs(runtime):
        pytest.skip("libtsan.so not found next to gcc: the toolchain cannot build the ThreadSanitizer library")
    p = subprocess.run(["make", "-C", CSRC, "tsan"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout[-3000:]
    p = subprocess.run([os.path.join(CSRC, "build", "tsan_host_forms")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    print(p.stdout[-3000:])
    assert p.returncode == 0 and "ThreadSanitizer" not in p.stdout and " 0 wrong outcomes" in p.stdout and " 0 (form, set) answers never seen" in p.stdout, p.stdout[-3000:]
