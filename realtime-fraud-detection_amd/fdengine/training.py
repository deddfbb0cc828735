"""Drop-in for the reference's ModelTrainer (ml/training/model_trainer.py): same constructor, attributes, method names,
result keys and written paths; the three tabular members — XGBoost, IsolationForest and the PyTorch MLP — are fitted,
saved, reloaded and scored on the engine.

What differs, on purpose:
* train_xgboost_model fits with FraudEngine.fit_gbdt (csrc/gbdt.hip) at the reference's parameters (max_depth 6,
  learning_rate 0.1, subsample 0.8, colsample_bytree 0.8, 100 estimators, random_state as the seed) and, as the
  reference does, watches the held-out split (eval_set, AUC per round in evals_result_). early_stopping_rounds and
  scale_pos_weight are attributes the reference leaves at XGBoost's defaults; so do these. The fit's
  arithmetic is the engine's own declared one: the file it writes is XGBoost 2.0.3 JSON that XGBoost and
  this engine load, but its trees are not the trees XGBoost would have grown.
* The synthetic frame has the reference's 33 feature columns, label rule and 5 % fraud rate, drawn vectorised from one
  numpy.random.Generator: the reference's per-row np.random stream (and so its exact rows) is not reproduced.
* The stratified 80 / 20 split is this module's own (no sklearn.model_selection needed).
* auc_score is the Mann-Whitney statistic over midranks of the engine's probabilities (equal to sklearn's
  roc_auc_score); feature_importance is the normalised mean gain per feature, XGBClassifier's default for gbtree.
* train_isolation_forest fits with FraudEngine.fit_iforest (csrc/iforest_fit.hip) at the reference's parameters (100
  estimators, contamination 0.05, random_state as the seed, normal transactions only). The fit's arithmetic is the
  engine's own declared one: the joblib file it writes is a scikit-learn IsolationForest that
  scikit-learn and this engine load, but its trees are not the trees scikit-learn's random stream would have grown.
  scikit-learn and joblib are needed for that file only; IsolationForest.fit never sees the training data.
  auc_score is taken from the engine's raw path-length sums: -decision_function is decreasing in them, so the
  midrank statistic is the reference's.
* train_graph_neural_model exists: the reference's docstring promises a GNN trainer and holds none, so nothing there
  writes pytorch/gnn_fraud_model.pth. It fits the registry's architecture (hidden_channels 64, num_layers 3, dropout
  0.1: an MLP 64 -> 64 -> 64 -> 2) with FraudEngine.fit_mlp (csrc/mlp_fit.hip) on the matrix as the
  serving side feeds it — padded with zeros to 64 columns and clipped to +-10 (EnsemblePredictor._prepare_features);
  the trainer's own 33 columns would not load into the 64-wide model — writes a plain state dict with torch.save,
  reloads it into the engine's MLP slot and scores the held-out split with the serving kernel.
"""
from __future__ import annotations

import json
import logging
import os
import time
from datetime import datetime
from typing import Any, Dict, Optional, Tuple

import numpy as np

from .forest import ForestArrays, load_isolation_forest_joblib, sklearn_iforest_from_forest, xgboost_doc_from_forest

ID_COLUMNS = ("is_fraud", "transaction_id", "user_id", "merchant_id")
XGB_PARAMS = dict(max_depth=6, learning_rate=0.1, subsample=0.8, colsample_bytree=0.8, n_estimators=100)
IFOREST_PARAMS = dict(n_estimators=100, contamination=0.05)
MLP_PARAMS = dict(hidden=64, n_layers=3, dropout=0.1)  # the registry's graph_neural hyperparameters
MLP_WIDTH = 64                                          # the scoring vector's width (_prepare_features)


def scoring_matrix(X) -> np.ndarray:
    """A feature matrix as the serving side hands it to the members: f32, padded with zeros (or cut) to 64 columns,
    clipped to [-10, 10] (EnsemblePredictor._prepare_features)."""
    X = np.asarray(X, dtype=np.float64)
    out = np.zeros((X.shape[0], MLP_WIDTH), np.float32)
    k = min(X.shape[1], MLP_WIDTH)
    out[:, :k] = np.clip(X[:, :k], -10.0, 10.0)
    return out


def roc_auc_midrank(y_true, score) -> float:
    """Area under the ROC curve as the Mann-Whitney U statistic over midranks (ties count half). Raises ValueError
    when only one class is present, as sklearn.metrics.roc_auc_score does."""
    y = np.asarray(y_true).astype(bool).reshape(-1)
    s = np.asarray(score, dtype=np.float64).reshape(-1)
    n1, n0 = int(y.sum()), int((~y).sum())
    if n1 == 0 or n0 == 0:
        raise ValueError("Only one class present in y_true. ROC AUC score is not defined in that case.")
    order = np.argsort(s, kind="stable")
    ss = s[order]
    start = np.r_[0, np.nonzero(ss[1:] != ss[:-1])[0] + 1]  # first place of each run of equal scores
    end = np.r_[start[1:], len(ss)]
    mid = (start + end + 1) / 2.0  # the mean of the 1-based places start + 1 .. end
    rank = np.empty(len(ss), np.float64)
    rank[order] = np.repeat(mid, end - start)
    return float((rank[y].sum() - n1 * (n1 + 1) / 2.0) / (float(n1) * float(n0)))


def gain_importance(fa: ForestArrays) -> np.ndarray:
    """XGBClassifier.feature_importances_ for gbtree (importance_type "gain"): per feature the mean loss change of
    its splits, normalised to sum 1 (all zeros when no tree split)."""
    gain = np.asarray(fa.meta["loss_changes"], np.float64)
    split = np.asarray(fa.left) != -1
    tot = np.bincount(np.asarray(fa.feature)[split], weights=gain[split], minlength=fa.num_feature)
    cnt = np.bincount(np.asarray(fa.feature)[split], minlength=fa.num_feature)
    mean = np.where(cnt > 0, tot / np.maximum(cnt, 1), 0.0)
    return mean / mean.sum() if mean.sum() > 0 else mean


def stratified_split(y, test_size: float, seed: int):
    """-> (train indices, test indices): per class, round(test_size * count) shuffled rows go to the test side."""
    rng = np.random.Generator(np.random.PCG64(seed))
    y = np.asarray(y)
    test = []
    for c in np.unique(y):
        idx = rng.permutation(np.nonzero(y == c)[0])
        test.append(idx[:int(round(test_size * len(idx)))])
    test = np.sort(np.concatenate(test))
    keep = np.ones(len(y), bool)
    keep[test] = False
    train = rng.permutation(np.nonzero(keep)[0])
    return train, rng.permutation(test)


class ModelTrainer:
    """Trains the fraud models on the engine."""

    def __init__(self, output_dir: str = "/app/models", engine=None):
        self.logger = logging.getLogger("model_trainer")
        self.output_dir = output_dir
        os.makedirs(output_dir, exist_ok=True)
        self.test_size = 0.2
        self.validation_size = 0.1
        self.random_state = 42
        # the XGBoost member's fit (FraudEngine.fit_gbdt): stop after this many rounds without a better held-out AUC
        # (None: never), the positive rows' gradient weight, and after train_xgboost_model the held-out curve
        self.early_stopping_rounds = None
        self.scale_pos_weight = 1.0
        self.evals_result_ = None
        # the MLP member's fit (FraudEngine.fit_mlp): epochs (default 20), rows per minibatch (default 256) and the
        # weight of the fraud class in the cross-entropy (default 1.0: unweighted, as the other members' defaults)
        self.mlp_epochs = 20
        self.mlp_batch_size = 256
        self.mlp_pos_weight = 1.0
        self._engine = engine
        self.logger.info(f"Model trainer initialized with output dir: {output_dir}")

    @property
    def engine(self):
        if self._engine is None:
            from .engine import FraudEngine
            self._engine = FraudEngine(0)
        return self._engine

    def prepare_training_data(self, data_path: Optional[str] = None) -> Tuple[np.ndarray, np.ndarray, np.ndarray,
                                                                             np.ndarray]:
        """-> (X_train, X_test, y_train, y_test) from a CSV (pandas) or the synthetic frame."""
        if data_path and os.path.exists(data_path):
            import pandas as pd
            self.logger.info(f"Loading training data from: {data_path}")
            df = pd.read_csv(data_path)
        else:
            self.logger.info("Generating synthetic training data")
            df = self._generate_synthetic_data()
        feature_columns = [c for c in df.columns if c not in ID_COLUMNS]
        X = df[feature_columns].values
        y = df["is_fraud"].values
        tr, te = stratified_split(y, self.test_size, self.random_state)
        self.logger.info(f"Training data prepared: {len(tr)} train, {len(te)} test samples")
        return X[tr], X[te], y[tr], y[te]

    def train_xgboost_model(self, X_train: np.ndarray, y_train: np.ndarray, X_test: np.ndarray,
                            y_test: np.ndarray) -> Dict[str, Any]:
        self.logger.info("Training XGBoost model...")
        start_time = time.time()
        eng = self.engine
        fa = eng.fit_gbdt(X_train, y_train, eval_set=(X_test, y_test), eval_metric="auc",
                          early_stopping_rounds=self.early_stopping_rounds, scale_pos_weight=self.scale_pos_weight,
                          random_state=self.random_state, **XGB_PARAMS)
        self.evals_result_ = fa.meta["evals_result"]
        model_path = os.path.join(self.output_dir, "xgboost", "fraud_classifier.json")
        os.makedirs(os.path.dirname(model_path), exist_ok=True)
        with open(model_path, "w") as f:
            json.dump(xgboost_doc_from_forest(fa), f)
        # score the held-out split with the file just written, as the serving side will
        slot = self._free_slot(eng)
        eng.load_xgboost_file(slot, model_path)
        try:
            y_pred_proba = eng.predict(slot, np.asarray(X_test, dtype=np.float32))
        finally:
            eng.unload_forest(slot)
        auc_score = roc_auc_midrank(y_test, y_pred_proba)
        training_time = time.time() - start_time
        results = {
            "model_type": "xgboost",
            "model_path": model_path,
            "auc_score": auc_score,
            "training_time_seconds": training_time,
            "feature_importance": dict(zip(range(X_train.shape[1]), gain_importance(fa))),
        }
        self.logger.info(f"XGBoost training completed in {training_time:.2f}s, AUC: {auc_score:.4f}")
        return results

    @staticmethod
    def _free_slot(eng) -> int:
        from . import _native as N
        for s in range(7, -1, -1):
            if s not in eng.forests and s not in (getattr(N, "FD_SLOT_LSTM", -1), getattr(N, "FD_SLOT_MLP", -1)):
                return s
        raise RuntimeError("no free forest slot to score the trained model in")

    def _generate_synthetic_data(self, n_samples: int = 10000):
        """The reference's 33 feature columns and label rule, one vectorised draw per column."""
        import pandas as pd
        rng = np.random.Generator(np.random.PCG64(self.random_state))
        n = n_samples

        def flag(p):
            return (rng.random(n) < p).astype(np.int64)

        amount = rng.lognormal(3, 1.5, n)
        cols = {
            "transaction_id": [f"tx_{i}" for i in range(n)],
            "user_id": [f"user_{v}" for v in rng.integers(1, 1000, n)],
            "merchant_id": [f"merchant_{v}" for v in rng.integers(1, 500, n)],
            "amount": amount,
            "amount_log": np.log1p(amount),
            "amount_percentile": rng.uniform(0, 100, n),
            "amount_zscore": rng.normal(0, 1, n),
            "hour_of_day": rng.integers(0, 24, n),
            "day_of_week": rng.integers(0, 7, n),
            "is_weekend": flag(0.3),
            "user_transaction_count_1h": rng.poisson(2, n),
            "user_transaction_count_24h": rng.poisson(10, n),
            "user_total_amount_24h": rng.lognormal(5, 1, n),
            "user_avg_amount": rng.lognormal(3, 1, n),
            "user_unique_merchants_24h": rng.poisson(3, n),
            "merchant_transaction_count_1h": rng.poisson(50, n),
            "merchant_fraud_rate": rng.beta(1, 10, n),
            "merchant_avg_amount": rng.lognormal(4, 1, n),
            "merchant_risk_score": rng.beta(2, 8, n),
            "device_risk_score": rng.beta(1, 9, n),
            "is_new_device": flag(0.2),
            "ip_risk_score": rng.beta(1, 9, n),
            "is_tor_ip": flag(0.01),
            "is_vpn_ip": flag(0.05),
            "velocity_score": rng.beta(2, 8, n),
            "amount_velocity_1h": rng.lognormal(2, 1, n),
            "transaction_velocity_5m": rng.poisson(1, n),
            "distance_from_home": rng.exponential(10, n),
            "location_risk_score": rng.beta(2, 8, n),
            "country_risk_score": rng.beta(3, 7, n),
            "timezone_mismatch": flag(0.1),
            "payment_method_risk": rng.beta(2, 8, n),
            "card_type_risk": rng.beta(2, 8, n),
            "is_crypto_merchant": flag(0.05),
            "is_gift_card_merchant": flag(0.1),
            "cross_border_transaction": flag(0.2),
        }
        score = (cols["merchant_fraud_rate"] * 0.3 + cols["device_risk_score"] * 0.2 + cols["ip_risk_score"] * 0.2
                 + cols["velocity_score"] * 0.15 + cols["location_risk_score"] * 0.15)
        score = score + 0.3 * ((cols["is_tor_ip"] == 1) | (cols["is_crypto_merchant"] == 1))
        score = score + 0.2 * ((cols["is_new_device"] == 1) & (amount > 1000))
        score = score + 0.1 * ((cols["hour_of_day"] < 6) | (cols["hour_of_day"] > 22))
        score = np.clip(score + rng.normal(0, 0.1, n), 0, 1)
        fraud = (score > 0.7).astype(np.int64)
        # hold the fraud rate at 5 %: flip random rows of the class in excess
        target = int(n * 0.05)
        have = int(fraud.sum())
        if have > target:
            fraud[rng.choice(np.nonzero(fraud == 1)[0], have - target, replace=False)] = 0
        elif have < target:
            fraud[rng.choice(np.nonzero(fraud == 0)[0], target - have, replace=False)] = 1
        cols["is_fraud"] = fraud
        df = pd.DataFrame(cols)
        self.logger.info(f"Generated {len(df)} synthetic transactions with {df['is_fraud'].sum()} fraud cases "
                         f"({df['is_fraud'].mean():.1%} fraud rate)")
        return df

    def train_isolation_forest(self, X_train: np.ndarray, y_train: np.ndarray, X_test: np.ndarray,
                               y_test: np.ndarray) -> Dict[str, Any]:
        """The engine fits the IsolationForest; scikit-learn and joblib only carry the file (ImportError without)."""
        import joblib
        self.logger.info("Training Isolation Forest model...")
        start_time = time.time()
        eng = self.engine
        X_normal = np.asarray(X_train)[np.asarray(y_train) == 0]  # normal transactions only
        fa = eng.fit_iforest(X_normal, seed=self.random_state, **IFOREST_PARAMS)
        model_path = os.path.join(self.output_dir, "sklearn", "isolation_forest.joblib")
        os.makedirs(os.path.dirname(model_path), exist_ok=True)
        joblib.dump(sklearn_iforest_from_forest(fa), model_path)
        # score the held-out split with the file just written, as the serving side will
        slot = self._free_slot(eng)
        eng.load_forest(slot, load_isolation_forest_joblib(model_path))
        try:
            _, raw = eng.predict(slot, np.asarray(X_test, dtype=np.float32), want_raw=True)
        finally:
            eng.unload_forest(slot)
        auc_score = roc_auc_midrank(y_test, -raw)  # shorter paths are more anomalous
        training_time = time.time() - start_time
        results = {
            "model_type": "isolation_forest",
            "model_path": model_path,
            "auc_score": auc_score,
            "training_time_seconds": training_time,
        }
        self.logger.info(f"Isolation Forest training completed in {training_time:.2f}s, AUC: {auc_score:.4f}")
        return results

    def train_graph_neural_model(self, X_train: np.ndarray, y_train: np.ndarray, X_test: np.ndarray,
                                 y_test: np.ndarray) -> Dict[str, Any]:
        """The registry's graph_neural member (model_type "pytorch"), fitted, written, reloaded and scored on the
        engine; torch only carries the file."""
        from .mlp import load_mlp_file, save_state_dict
        self.logger.info("Training graph_neural (MLP) model...")
        start_time = time.time()
        eng = self.engine
        w = eng.fit_mlp(scoring_matrix(X_train), np.asarray(y_train), epochs=self.mlp_epochs,
                        batch_size=self.mlp_batch_size, pos_weight=self.mlp_pos_weight, seed=self.random_state,
                        **MLP_PARAMS)
        model_path = os.path.join(self.output_dir, "pytorch", "gnn_fraud_model.pth")
        os.makedirs(os.path.dirname(model_path), exist_ok=True)
        save_state_dict(w, model_path)
        # score the held-out split with the file just written, as the serving side will (an engine has one MLP slot)
        if getattr(eng, "mlp_info", None):
            raise RuntimeError("the engine's MLP slot is in use: train on an engine that serves no MLP")
        eng.load_mlp(load_mlp_file(model_path))
        try:
            y_pred_proba = eng.mlp_predict(scoring_matrix(X_test))
        finally:
            eng.unload_mlp()
        auc_score = roc_auc_midrank(y_test, y_pred_proba)
        training_time = time.time() - start_time
        results = {
            "model_type": "graph_neural",
            "model_path": model_path,
            "auc_score": auc_score,
            "training_time_seconds": training_time,
            "loss_curve": [float(v) for v in w.meta["loss_curve"]],
        }
        self.logger.info(f"graph_neural training completed in {training_time:.2f}s, AUC: {auc_score:.4f}")
        return results

    def save_training_metadata(self, results: Dict[str, Any]) -> None:
        metadata = {
            "timestamp": datetime.now().isoformat(),
            "training_results": results,
            "configuration": {
                "test_size": self.test_size,
                "validation_size": self.validation_size,
                "random_state": self.random_state,
            },
        }
        metadata_path = os.path.join(self.output_dir, "training_metadata.json")
        with open(metadata_path, "w") as f:
            json.dump(metadata, f, indent=2, default=float)
        self.logger.info(f"Training metadata saved to: {metadata_path}")
