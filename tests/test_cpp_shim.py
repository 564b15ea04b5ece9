"""CPU suite: include/rsbwt_gpubwt.hpp compiles against the reference's own headers and links with
the reference's unmodified src/bwt/query.cpp + librsbwt.so -- the drop-in claim of INTEGRATION.md.
build() compiles that program (oracle/shim_batch.cpp) into oracle/_ref/shim_batch by oracle/Makefile's
`ref` recipe, where the reference's sources are at hand; skipped where it could not."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "oracle", "_ref", "shim_batch")


@pytest.mark.skipif(not os.path.exists(EXE), reason="oracle/_ref/shim_batch not built: the reference's sources were not at hand")
def test_shim_builds_against_reference_and_fails_loudly_without_gpu(rsb, tmp_path):
    bwt = tmp_path / "t.bwt"
    rsb.synth_popbwt(str(bwt), None, seed=1, genome_len=500, haplotypes=2, snp_rate=0.01, read_len=30,
                     coverage=2.0)
    p = subprocess.run([EXE, str(bwt), "ACGT"], capture_output=True, text=True)
    if rsb.lib().rsbwt_device_count() == 0:
        assert p.returncode == 3 and "no CPU fallback" in p.stdout
    else:
        a = p.stdout.split()
        assert p.returncode == 0 and a[0] == a[2] and a[1] == a[3]
