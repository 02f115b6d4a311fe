"""The 54 seeded cases of tests/coherence_cases.py on the GPU against tests/coherence_ref.py: every instantiation of
k_detect_coh three times, with rows per segment 8 ... 72, one to three segments per call into a handle that may hold
one more, batches collected with a lag over one to three buffer sets, one or two antennas that carry their OWN data
(each held to the reference of its own stream: a wrong antenna stride into the spectra, the row weights, the bandpass
or the codes shows), injection, keep_ave on and off, and per antenna one content edge (a dead pol, a saturated
stretch, dropped frames, a row flagged whole in both pols or in one, a first segment of code 0 or with one pol dead).
tests/test_coherence_cases_cpu.py holds the reference's AA / BB half to the oracle on the same inputs.

Codes: every byte equal, samples whose plane is NaN included (the quantiser of a NaN is orc_sel_and_dig_*'s).  Planes
and the final bandpass state: the same bits where the reference is not NaN, NaN where it is."""
import numpy as np
import pytest

import coherence_cases as CC
import coherence_ref as CR
from helpers import libpb
from test_gpu_coherence_matrix import NAMES, run_calls

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("seed", range(CC.NCASES))
def test_random_coherence_configuration(oracle, seed):
    c = CC.case(seed)
    lp = libpb()
    R, mode, nbit, nseg, nb = c["R"], c["rfi_mode"], c["nbit"], c["nseg"], c["nb"]
    got, bps = run_calls(lp, c["datas"], R, mode, nbit, calls=(nseg,) * nb, max_seg=c["max_seg"], nsets=c["nsets"],
                         lag=c["lag"], keep_ave=c["keep_ave"], inject=c["inject"])
    delays = oracle.set_frb_delays(80.0, R) if c["inject"] else None
    what = CC.describe(c)
    bad = []
    for a in range(c["nant"]):
        ref = CR.run(oracle, c["datas"][a], R, mode, nbit, delays, 1 if c["inject"] else 0)
        nt = nseg * nb * R // 8
        for st in CC.streams(mode):
            rc, rp = ref[st]
            codes, planes = got[a][st]
            assert codes.size == rc.size, (what, a, NAMES[st], codes.size, rc.size)
            gc, rcv = codes.reshape(nt, 4, -1), rc.reshape(nt, 4, -1)
            for k, pr in enumerate(CC.PRODUCTS):
                nd = int((gc[:, k] != rcv[:, k]).sum())
                if nd:
                    bad.append("antenna %d, %s stream, %s codes: %d of %d bytes differ" % (a, NAMES[st], pr, nd, rcv[:, k].size))
                if c["keep_ave"]:
                    nd = CC.f32_diff(planes[:, k], rp[:, k])
                    if nd:
                        bad.append("antenna %d, %s stream, %s plane: %d of %d values differ" % (a, NAMES[st], pr, nd, rp[:, k].size))
            for pol, pr in enumerate(CC.PRODUCTS[:2]):
                nd = CC.f32_diff(bps[a][st][pol], ref.state.bp[st][pol])
                if nd:
                    bad.append("antenna %d, %s stream, bandpass state of %s: %d of %d values differ"
                               % (a, NAMES[st], pr, nd, ref.state.bp[st][pol].size))
    assert not bad, "case %s:\n  %s" % (what, "\n  ".join(bad))
