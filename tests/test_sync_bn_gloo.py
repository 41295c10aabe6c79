"""CPU, two and three processes over gloo with interpreted kernels: a small stack of the package's own layers (Conv2d ->
SyncBatchNorm2d with a residual and ReLU -> Conv2d -> SyncBatchNorm2d with ELU; 6 and 8 channels, 8 x 8 maps) with unequal per-rank
batches, GradAllReducer around it, three training steps with a plain SGD update (the last with two backward() calls on the shared
trunk, as trainer.train_step makes them) against the float64 full-batch oracle (tests/sync_bn_cases.py).  One spawn per
configuration, shared by the tests below; every worker runs under a time limit and a failed rank ends the others."""
import pytest
import torch

import bn_bitmask_cases as BM
import emu
import sync_bn_cases as SC

BATCHES = [(2, 1), (1, 1, 2)]
IDS = ["2 ranks", "3 ranks"]


@pytest.fixture(scope="module", autouse=True)
def _emu():
    if torch.cuda.is_available():
        pytest.skip("GPU present: the interpreter build is exercised on the CPU machines")
    emu.install()           # (builds the interpreter library once, before the workers load it)


@pytest.mark.parametrize("batches", BATCHES, ids=IDS)
def test_matches_full_batch_oracle(batches):
    """(a), (e): outputs, input gradients, averaged parameter gradients and running buffers of all three steps under the K rule
    (end to end: K_STACK, see tests/sync_bn_cases.py)"""
    rows = SC.gloo_compare(batches)
    SC.stack_worst(rows)
    bad = [r for r in rows if not r[6] <= SC.K_STACK]
    assert not bad, "error against float64 above %g times the fp32 reference's: %s" % (SC.K_STACK, bad)


@pytest.mark.parametrize("batches", BATCHES, ids=IDS)
def test_statistics_bitwise_equal_on_all_ranks(batches):
    """(b): after each step running_mean / running_var and the saved mean / invstd of both BatchNorms, bit for bit"""
    runs = SC.gloo_run(batches)
    for step in range(SC.GLOO_STEPS):
        recs = [r["steps"][step] for r in runs]
        assert len(recs[0]["saved"]) == 2, "one statistics exchange per BatchNorm and step"
        for r in range(1, len(batches)):
            for k in SC.BUFFERS:
                BM.same_bits(recs[r]["bufs"][k], recs[0]["bufs"][k], "step %d rank %d %s" % (step, r, k))
            assert len(recs[r]["saved"]) == 2
            for i in range(2):
                for j, what in enumerate(("mean", "invstd")):
                    BM.same_bits(recs[r]["saved"][i][j], recs[0]["saved"][i][j], "step %d rank %d BatchNorm %d saved %s" % (step, r, i, what))


def test_unconverted_model_misses_the_oracle():
    """(c): the same script without convert_sync_batchnorm normalises over each rank's own samples and misses the oracle"""
    rows = SC.gloo_compare(BATCHES[0], convert=False)
    bad = {(r[1], r[2]) for r in rows if not r[6] <= SC.K_STACK}
    assert any(t == "out" for _, t in bad) and any(t == "dx" for _, t in bad) and any(t.startswith("bn1.running") for _, t in bad), bad
    assert all(r["steps"][0]["gathers"] == 0 for r in SC.gloo_run(BATCHES[0], convert=False))


@pytest.mark.parametrize("batches", BATCHES, ids=IDS)
def test_collectives_counted(batches):
    """(d): a module in eval() issues no collective; in training each BatchNorm gathers once per forward and once per backward()"""
    for r in SC.gloo_run(batches):
        assert r["eval_gathers"] == 0
        assert [s["gathers"] for s in r["steps"]] == [4, 4, 6]
