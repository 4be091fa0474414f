"""model-predict-2d: a trained model and a data volume file to a label volume.

    python -m volume_segmantics_amd.scripts.predict_2d_model MODEL.pytorch DATA.h5 [--data_dir DIR]

Reads ``DIR/volseg-settings/2d_model_predict_settings.yaml``; writes ``DIR/<date>_<stem of DATA>_2d_model_vol_pred.h5``."""
from __future__ import annotations

import logging

from ..data import get_settings_data
from ..utilities import arg_parsing
from ..utilities import config as cfg


def main(argv=None) -> None:
    logging.basicConfig(level=logging.INFO, format=cfg.LOGGING_FMT, datefmt=cfg.LOGGING_DATE_FMT)
    args = arg_parsing.get_2d_prediction_parser().parse_args(argv)
    root = arg_parsing.root_path(args)
    model_path, data_path = getattr(args, cfg.MODEL_PTH_ARG), getattr(args, cfg.PREDICT_DATA_ARG)
    settings = get_settings_data(root / cfg.SETTINGS_DIR / cfg.PREDICTION_SETTINGS_FN)
    from ..model.operations.vol_seg_prediction_manager import VolSeg2DPredictionManager
    manager = VolSeg2DPredictionManager(str(model_path), data_path, settings)
    manager.predict_volume_to_path(arg_parsing.prediction_output_path(root, data_path))


if __name__ == "__main__":
    main()
