"""The fused kernel over the dense chunk stream of the contracted forests (csrc/ensemble_plan.hip dense_layout_host,
walk_dense, owner_sum_dense; engine option ensemble_contract 3: bundles of consecutive trees, 4: the chunk's trees
sorted by depth), with the twin scheme of test_gpu_ensemble_contract.py at the same sizes: a pipelined engine scores
split rows and compact 64-B rows through the dense chunks, a serial twin scores the full 64-wide vectors over the
uncontracted forests — outputs, model probabilities and end state bit-identical, in the wide and the compact chunk
geometry. Batches of 33,000 and 33,001 rows reach the fused kernel (128 tiles of 256 at least; the last tile partial),
a 1,000-row batch between them takes the latency path. The engine's node-step and chunk counters are held to
fd_dense_layout_host's layout of each forest."""
import numpy as np
import pytest

import dense_cases as DC
import test_gpu_ensemble_contract as B
from fdengine import FraudEngine, iforest_from_sklearn, synth, xgboost_from_json_doc
from fdengine._native import TXN_FIELDS
from fdengine.engine import dense_layout_host

pytestmark = pytest.mark.gpu

CUTS = B.CUTS


@pytest.fixture(scope="module")
def world():
    """test_gpu_ensemble_contract.py's population, stream and models, and the two forests of test_dense_host.py whose
    chunks end at the bundle cap and at the byte cap"""
    import torch
    pop = synth.population(20000, 5000, seed=17)
    tx = synth.txn_stream(pop, CUTS[-1] + 4096, seed=18)
    warm = FraudEngine(0)
    try:
        U, M = pop["users"], pop["merchants"]
        warm.state_init(1 << 17, 1, 16)
        warm.load_users(U["key"], U["avg_amount"], U["account_age_days"], U["device_fp"])
        warm.load_merchants(M["fraud_rate"], M["risk_multiplier"])
        X = warm.features({k: v[:16384] for k, v in tx.items()})[-8192:]
    finally:
        warm.close()
    ifm = iforest_from_sklearn(synth.isolation_forest(X.astype(np.float64), n_estimators=20))
    models = {"mixed": (xgboost_from_json_doc(synth.xgboost_doc(50, 8, 64, X, seed=3, p_leaf=0.1)), ifm),
              "depth3": (xgboost_from_json_doc(synth.xgboost_doc(30, 3, 64, X, seed=4)), ifm)}
    c = xgboost_from_json_doc(synth.xgboost_doc(30, 5, 64, X, seed=5, p_leaf=0.2))
    six = slice(0, int(c.offsets[6]))  # the first six trees: every split on a constant slot, both directions taken
    c.feature[six] = B.CONST[np.arange(six.stop) % len(B.CONST)]
    c.threshold[six] = 0.25
    models["six_constant"] = (c, ifm)
    d = DC.on_varying(xgboost_from_json_doc(synth.xgboost_doc(30, 4, 64, X, seed=6)))  # perfect trees, varying slots
    di = DC.on_varying(xgboost_from_json_doc(synth.xgboost_doc(16, 4, 64, X, seed=7)))
    models["nothing_to_prune"] = (d, DC.as_iforest(di, 8))
    models["shallow200"] = (DC.shallow200(X), ifm)
    models["deep_then_shallow"] = (DC.deep_then_shallow(X), ifm)
    dev = {f: torch.from_numpy(np.ascontiguousarray(tx[f][:CUTS[-1]])).cuda() for f in TXN_FIELDS}
    torch.cuda.synchronize()
    return dict(pop=pop, tx=tx, dev=dev, models=models, ref={})


@pytest.mark.timeout(120)
@pytest.mark.parametrize("chunks", [1, 2], ids=["wide", "compact_chunks"])
@pytest.mark.parametrize("contract", [3, 4], ids=["consecutive", "sorted"])
@pytest.mark.parametrize("name", ["mixed", "depth3", "six_constant", "nothing_to_prune", "shallow200",
                                  "deep_then_shallow"])
def test_dense_walk_matches_the_serial_twin(world, name, contract, chunks):
    import torch
    batches, end, steps = B._reference(world, name)
    xgb, ifm = world["models"][name]
    params = FraudEngine.blend_params(*B._blend())
    lays = [dense_layout_host(fa, wide=chunks == 1, mode=contract)["info"] for fa in (xgb, ifm)]
    want_steps, want_chunks = sum(i.node_steps for i in lays), sum(i.n_chunks for i in lays)
    for rows in (2, 1):  # split rows, compact 64-B rows
        pip = B._engine(world["pop"], xgb, ifm)
        try:
            pip.set_stream(torch.cuda.current_stream().cuda_stream)
            for k, v in (("ensemble_contract", contract), ("ensemble_chunks", chunks), ("compact_vectors", rows)):
                pip.set_option(k, v)
            got = []
            for a, b in zip(CUTS[:-1], CUTS[1:]):
                n = b - a
                outs = [torch.empty(n, dtype=t, device="cuda")
                        for t in (torch.float64, torch.float64, torch.uint8, torch.uint8)]
                mp = torch.empty((2, n), dtype=torch.float64, device="cuda")
                pip.score_batch_pipelined(params, [0, 1], {f: t[a:b].data_ptr() for f, t in world["dev"].items()}, n,
                                          *[o.data_ptr() for o in outs], model_probs_ptr=mp.data_ptr())
                got.append((outs, mp))
            torch.cuda.synchronize()
            for (outs, mp), (w_outs, w_mp, _) in zip(got, batches):
                np.testing.assert_array_equal(mp.cpu().numpy(), w_mp)
                for x, y in zip(outs, w_outs):
                    np.testing.assert_array_equal(x.cpu().numpy(), y)
            assert pip.counter("pipelined_compact_batches") == 2  # the two large batches: the fused kernel's rows
            launches, walked = pip.counter("ensemble_contracted_launches"), pip.counter("ensemble_node_steps_per_txn")
            dense = pip.counter("ensemble_dense_chunks")
            print(f"{name} contract={contract} chunks={chunks} rows={rows}: contracted launches {launches}, node steps "
                  f"per txn {walked} (layout {want_steps}, own depths {steps['own']}, full {steps['full']}), dense "
                  f"chunks {dense} (layout {want_chunks})")
            if name == "nothing_to_prune":  # nothing shortened: the padded chunks and the fixed-depth kernel ran
                assert steps["own"] == steps["full"] == want_steps
                assert launches == 0 and walked == steps["full"] and dense == 0
            else:
                assert launches == 2 and walked == want_steps < steps["full"] and dense == want_chunks
                assert steps["own"] <= want_steps
            nxt = {k: v[CUTS[-1]:CUTS[-1] + 4096] for k, v in world["tx"].items()}
            np.testing.assert_array_equal(pip.features(nxt), end)
        finally:
            pip.close()
