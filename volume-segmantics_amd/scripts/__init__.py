"""The two commands: ``python -m volume_segmantics_amd.scripts.train_2d_model`` (model-train-2d) and
``python -m volume_segmantics_amd.scripts.predict_2d_model`` (model-predict-2d)."""
