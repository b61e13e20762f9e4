"""The complete driver on interleaved samples: the `main` call sequence (fhe-linformer_amd/linformer.py, src/main.cpp:145-475 with its
8 bootstraps) at the headline configuration of bench.py - N = 2^16, 28+7 limbs - with TWO samples in every ciphertext (slot stride 2:
the 32768 physical slots are the ring's full packing, so bootstrapping runs unpacked with two EvalMods).  Each lane's logits are
compared with the same operation sequence in the clear (oracle/circuit_sim.py) on that lane's own sample.
As long as the headline forward test, so behind FHELIN_SLOW_TESTS=1 like the other long runs (a recorded run:
profiles/interleave_forward_test.txt)."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
LOGIT_TOL = 1.2e-2          # tests/test_forward_gpu.py


@pytest.mark.skipif(not os.environ.get("FHELIN_SLOW_TESTS"), reason="a whole forward pass at N=2^16 with two engines' worth of keys; "
                    "FHELIN_SLOW_TESTS=1 runs it (recorded: profiles/interleave_forward_test.txt)")
def test_interleaved_forward_matches_plaintext_circuit_per_lane(fa):
    from fhe_linformer_amd import linformer as lf
    from oracle import plain_forward as pf, circuit_sim as cs
    S, stride = 129, 2
    w = pf.synthetic_model(1234)
    xs = [pf.synthetic_tokens(S, 4321 + i) for i in range(stride)]
    refs = []
    for x in xs:
        sim = cs.SlotSimController()
        refs.append(lf.logits_from_slots(lf.forward(sim, w, *pf.client_inputs(w, x), None, "main")))
    assert np.max(np.abs(refs[0] - refs[1])) > 10 * LOGIT_TOL          # the two samples' logits differ: a lane swap cannot pass
    eng = fa.Engine("bench", seed=11, n_q=28, n_p=-1, interleave=stride)
    try:
        eng.keygen()
        eng.gen_relin_key()
        eng.gen_rotation_keys(fa.circuit_rotation_indices())
        eng.bootstrap_setup(3, 3, 16384)
        ctl = lf.GpuController(eng)
        enc = lf.ingest_sample(ctl, w, xs)
        out = lf.forward_encrypted(ctl, w, enc, None, "main")
        assert ctl.n_boot == sim.n_boot == 3 + -(-(S + 1) // 32)
        lanes = ctl.decrypt_lanes(out)
        assert lanes.shape == (stride, 16384)
        for i in range(stride):
            lg = lf.logits_from_slots(lanes[i])
            err = np.max(np.abs(lg - refs[i]))
            print(f"interleaved main bench S={S} lane {i}: logits {err:.2e} (< {LOGIT_TOL:.0e})")
            assert err < LOGIT_TOL, (i, err)
            top2 = np.sort(refs[i])[-2:]
            if top2[1] - top2[0] > 4e-2:
                assert int(np.argmax(lg)) == int(np.argmax(refs[i])), i
        assert out.info()["ell"] >= 2 and out.info()["slots"] == 16384
    finally:
        eng.close()
