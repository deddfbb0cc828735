"""The fused kernel's variable-depth walk over forests contracted against the compact vector's constant slots
(csrc/ensemble_plan.hip contract_forest_host, csrc/ensemble.hip walk_ens_var; engine option ensemble_contract),
with the twin scheme of test_gpu_pipeline.py: a pipelined engine scores split rows (and compact 64-B rows) through
the contracted chunks, a serial twin scores the full 64-wide vectors with score_batch_device over the uncontracted forests — outputs, model
probabilities and end state bit-identical at ensemble_contract 1 (each tree to its wave's deepest), 2 (to its own
depth) and 0, in the wide and the compact chunk layout. Batches of 33,000 and 33,001 rows reach the fused kernel
(128 tiles of 256 at least; the last tile partial), a 1,000-row batch between them takes the latency path. The twin's
probabilities are held to the CPU oracle's on the twin's own vectors (1e-5), and the engine's node-step counter to
the CPU contraction's depths."""
import numpy as np
import pytest

import oracle
from fdengine import ForestArrays, FraudEngine, iforest_from_sklearn, synth, xgboost_from_json_doc
from fdengine import _native as N
from fdengine._native import TXN_FIELDS
from fdengine.engine import contract_forest_host, pack_forest_host

pytestmark = pytest.mark.gpu

VARYING = np.array([0, 1, 5, 6, 7, 14, 15, 16, 17, 19, 21, 23, 26, 27, 31, 32, 41, 42, 43, 44, 45, 46], np.int32)
CONST = np.array([f for f in range(64) if f not in set(VARYING.tolist())], np.int32)
CUTS = [0, 33000, 34000, 67001]
NAMES = ["xgboost_primary", "isolation_forest"]


def _blend():
    from oracle import scoring_ref as S
    w = S.normalized_weights({"xgboost_primary": 0.4, "isolation_forest": 0.05})
    return [w[k] for k in NAMES], [S.CONF_MULT[k] for k in NAMES]


def _engine(pop, xgb, ifm):
    U, M = pop["users"], pop["merchants"]
    eng = FraudEngine(0)
    eng.state_init(1 << 17, 1, 16)
    eng.load_users(U["key"], U["avg_amount"], U["account_age_days"], U["device_fp"])
    eng.load_merchants(M["fraud_rate"], M["risk_multiplier"])
    eng.load_forest(0, xgb)
    eng.load_forest(1, ifm)
    return eng


def _as_iforest(fa, seed):
    """the trees of an XGBoost-shaped forest as an IsolationForest (sklearn's comparison, f64 path-length leaves)"""
    rng = np.random.default_rng(seed)
    return ForestArrays(kind=N.FD_FOREST_SKLEARN_IFOREST, num_feature=64, offsets=fa.offsets, left=fa.left,
                        right=fa.right, feature=fa.feature, threshold=fa.threshold,
                        default_left=np.zeros_like(fa.default_left), leaf_value=rng.uniform(1.0, 9.0, len(fa.left)),
                        if_offset=-0.5, if_denominator=fa.n_trees * 10.24)


@pytest.fixture(scope="module")
def world():
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
    c.feature[six] = CONST[np.arange(six.stop) % len(CONST)]
    c.threshold[six] = 0.25
    models["six_constant"] = (c, ifm)
    d = xgboost_from_json_doc(synth.xgboost_doc(30, 4, 64, X, seed=6))  # perfect trees, varying slots only
    d.feature = VARYING[d.feature % len(VARYING)]
    di = xgboost_from_json_doc(synth.xgboost_doc(16, 4, 64, X, seed=7))
    di.feature = VARYING[di.feature % len(VARYING)]
    models["nothing_to_prune"] = (d, _as_iforest(di, 8))
    dev = {f: torch.from_numpy(np.ascontiguousarray(tx[f][:CUTS[-1]])).cuda() for f in TXN_FIELDS}
    torch.cuda.synchronize()
    return dict(pop=pop, tx=tx, dev=dev, models=models, ref={})


def _reference(world, name):
    """the serial twin, once per model: every batch's outputs, model probabilities and 64-wide vectors, and the end
    state; its probabilities against the oracle forests on those vectors"""
    import torch
    if name in world["ref"]:
        return world["ref"][name]
    xgb, ifm = world["models"][name]
    w, mults = _blend()
    params = FraudEngine.blend_params(w, mults)
    ref = _engine(world["pop"], xgb, ifm)
    try:
        ref.set_stream(torch.cuda.current_stream().cuda_stream)
        batches = []
        for a, b in zip(CUTS[:-1], CUTS[1:]):
            n = b - a
            outs = [torch.empty(n, dtype=t, device="cuda") for t in (torch.float64, torch.float64, torch.uint8, torch.uint8)]
            vec = torch.empty((n, 64), dtype=torch.float32, device="cuda")
            mp = torch.empty((2, n), dtype=torch.float64, device="cuda")
            ref.score_batch_device(params, [0, 1], {f: t[a:b].data_ptr() for f, t in world["dev"].items()}, n,
                                   *[o.data_ptr() for o in outs], vec_ptr=vec.data_ptr(), model_probs_ptr=mp.data_ptr())
            torch.cuda.synchronize()
            batches.append(([o.cpu().numpy() for o in outs], mp.cpu().numpy(), vec.cpu().numpy()))
        nxt = {k: v[CUTS[-1]:CUTS[-1] + 4096] for k, v in world["tx"].items()}
        end = ref.features(nxt)
    finally:
        ref.close()
    for outs, mp, V in batches:
        px, _, _ = oracle.xgb_predict(xgb, V)
        pi, _, _ = oracle.iforest_predict(ifm, V)
        assert np.abs(mp[0] - px).max() <= 1e-5 and np.abs(mp[1] - pi).max() <= 1e-5
        fp, conf, dec, risk = oracle.blend_weighted(np.stack([mp[0], mp[1]]), w, mults)
        np.testing.assert_array_equal(outs[0], fp)
        np.testing.assert_array_equal(outs[1], conf)
    steps = {}
    cx, dx, _ = contract_forest_host(xgb)
    ci, di, _ = contract_forest_host(ifm)
    D = max(pack_forest_host(xgb)[2].depth, pack_forest_host(ifm)[2].depth)
    steps["own"] = int(dx.sum() + di.sum())
    # per wave: a chunk's trees go to four tree groups in order, each tree walked to the deepest of its group's
    for lay, chs in ((1, (24, 16)), (2, (20, 12))):
        steps["wave", lay] = sum(int(max(d[g:g + ch // 4])) * len(d[g:g + ch // 4])
                                 for d, ch in ((dx, chs[0]), (di, chs[1])) for g in range(0, len(d), ch // 4))
    steps["full"] = (xgb.n_trees + ifm.n_trees) * D
    world["ref"][name] = (batches, end, steps)
    return world["ref"][name]


@pytest.mark.timeout(120)
@pytest.mark.parametrize("chunks", [1, 2], ids=["wide", "compact_chunks"])
@pytest.mark.parametrize("contract", [1, 0, 2], ids=["per_wave", "off", "per_tree"])
@pytest.mark.parametrize("name", ["mixed", "depth3", "six_constant", "nothing_to_prune"])
def test_contracted_walk_matches_the_serial_twin(world, name, contract, chunks):
    import torch
    batches, end, steps = _reference(world, name)
    xgb, ifm = world["models"][name]
    params = FraudEngine.blend_params(*_blend())
    for rows in (2, 1):  # split rows, compact 64-B rows
        pip = _engine(world["pop"], xgb, ifm)
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
            print(f"{name} contract={contract} chunks={chunks} rows={rows}: contracted launches {launches}, node steps "
                  f"per txn {walked} (own depths {steps['own']}, full {steps['full']}), pruned "
                  f"{pip.counter('ensemble_nodes_pruned')}")
            if name == "nothing_to_prune":
                assert steps["own"] == steps["full"]
            if contract == 0 or name == "nothing_to_prune":  # the uncontracted path ran
                assert launches == 0 and walked == steps["full"]
            elif contract == 2:  # the CPU contraction's sum of depths
                assert launches == 2 and walked == steps["own"] < steps["full"]
                assert pip.counter("ensemble_nodes_pruned") > 0
            else:  # every tree to the deepest of its wave's
                assert launches == 2 and walked == steps["wave", chunks] < steps["full"]
                assert pip.counter("ensemble_nodes_pruned") > 0
            nxt = {k: v[CUTS[-1]:CUTS[-1] + 4096] for k, v in world["tx"].items()}
            np.testing.assert_array_equal(pip.features(nxt), end)
        finally:
            pip.close()
