"""fdengine — MI355X-native drop-in for the fraud-scoring hot path of
AjayAlluri/realtime-fraud-detection (windowed features -> XGBoost + IsolationForest -> blend).

Host side of libfdengine.so (HIP/gfx950, C-ABI in include/fdengine.h). Importing this package
loads the native library and fails loudly if it is missing: there is no CPU fallback.
"""
from . import _native  # noqa: F401  (loads libfdengine.so or raises ImportError)
from .engine import (FraudEngine, device_count, gbdt_cuts_host, gbdt_fit_ref_host,  # noqa: F401
                     gbdt_grow_tree_ref_host, gbdt_metric_ref_host, iforest_fit_grow_tree_ref_host,
                     iforest_fit_ref_host, iforest_fit_sample_ref_host, pack_forest_host, pack_forest_sparse_host, shap_paths_host,
                     shap_ref_host)
from .forest import (ForestArrays, UnsupportedModel, forest_from_sklearn_classifier,  # noqa: F401
                     iforest_from_sklearn, load_isolation_forest_joblib, load_xgboost_json,
                     sklearn_iforest_from_forest, truncate_forest, xgboost_doc_from_forest,
                     xgboost_from_json_doc)
from .mlp import (MlpWeights, mlp_fit_batch_host, mlp_fit_ref_host, mlp_grad_ref_host,  # noqa: F401
                  save_state_dict)

__all__ = ["FraudEngine", "ForestArrays", "UnsupportedModel", "device_count", "forest_from_sklearn_classifier",
           "gbdt_cuts_host", "gbdt_fit_ref_host", "gbdt_grow_tree_ref_host", "gbdt_metric_ref_host",
           "iforest_fit_grow_tree_ref_host", "iforest_fit_ref_host", "iforest_fit_sample_ref_host",
           "iforest_from_sklearn", "load_isolation_forest_joblib", "load_xgboost_json", "MlpWeights", "mlp_fit_batch_host", "mlp_fit_ref_host", "mlp_grad_ref_host",
           "pack_forest_host", "pack_forest_sparse_host",
           "save_state_dict", "shap_paths_host", "shap_ref_host", "sklearn_iforest_from_forest", "truncate_forest",
           "xgboost_doc_from_forest", "xgboost_from_json_doc"]
