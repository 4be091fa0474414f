"""model-evaluate-2d: how good is a segmentation?  Scores a predicted label volume against a labelled one.

    python -m volume_segmantics_amd.scripts.evaluate_2d_model MODEL.pytorch DATA.h5 --labels LABELS.h5 [--data_dir DIR]
    python -m volume_segmantics_amd.scripts.evaluate_2d_model --prediction PRED.h5 --labels LABELS.h5 [--data_dir DIR]

The first form reads ``DIR/volseg-settings/2d_model_predict_settings.yaml``, predicts, writes the label volume to
``DIR/<date>_<stem of DATA>_2d_model_vol_pred.h5`` as the predict command does, and scores it.  The second takes no model: it scores
an existing label volume (one the reference wrote, for instance) and also runs on a host without a GPU; the class count is then the
number of distinct values over both files, class ``i`` being the ``i``-th of them in ascending order.  Both log the per-class table
and write ``<stem>_scores.csv`` and ``<stem>_scores.json`` beside the prediction's name under ``DIR`` (``<stem>_scores_per_slice.csv``
too with the settings key ``evaluation_per_slice: true``; ``<stem>_surface_scores.csv`` and ``<stem>_surface_scores.json`` - Hausdorff
distances, average symmetric surface distance, surface Dice - with ``evaluation_surface_distances: true``; ``<stem>_object_scores.csv``,
``<stem>_object_scores.json`` and ``<stem>_object_matches.csv`` - objects found, split, merged and invented, panoptic quality, variation
of information - with ``evaluation_object_scores: true``)."""
from __future__ import annotations

import logging

import numpy as np

from ..utilities import arg_parsing
from ..utilities import config as cfg


def _score_existing(root, pred_path, labels_path, settings) -> None:
    from ..utilities import base_data_utils as utils
    from ..utilities import evaluation as ev

    hdf5_path = getattr(settings, "data_hdf5_path", "/data")
    pred, _ = utils.get_numpy_from_path(pred_path, internal_path=hdf5_path)
    truth, _ = utils.get_numpy_from_path(labels_path, internal_path=getattr(settings, "seg_hdf5_path", hdf5_path))
    if pred.shape != truth.shape:
        raise ValueError(f"the prediction has shape {pred.shape} but the label volume has shape {truth.shape}")
    ignore = getattr(settings, "evaluation_ignore_label", None)
    values = np.union1d(np.unique(pred), np.unique(truth)).astype(np.int64)
    if ignore is not None:
        values = values[values != int(ignore)]
    # both files hold label VALUES: the prediction goes through the same value -> class map as the truth
    # (a prediction voxel that carries the ignore value has no class: 255, which is reported as invalid unless its truth is ignored)
    wide = pred.astype(np.int64)
    pos = np.clip(np.searchsorted(values, wide), 0, max(len(values) - 1, 0))
    pred_classes = np.where(values[pos] == wide, pos, 255).astype(np.uint8 if len(values) <= 255 else np.int64)
    scores, dropped, slab_dice = ev.evaluate_label_volumes(pred_classes, truth, len(values), label_values=values, ignore_label=ignore,
                                                           per_slice=bool(getattr(settings, "evaluation_per_slice", False)))
    logging.info("Scores against the label volume:\n" + ev.score_table(scores, values))
    ev.write_scores(root / pred_path.stem, scores, dropped, values, slab_dice)
    from ..utilities import surface_distance as sd
    if sd.surface_settings(settings)[0]:
        sd.evaluate_surface_distances(pred_classes, truth, len(values), settings, label_values=values, ignore_label=ignore,
                                      stem=root / pred_path.stem)
    from ..utilities import object_scores as obs
    if obs.object_scores_asked(settings):
        obs.evaluate_objects(pred_classes, truth, len(values), settings, label_values=values, ignore_label=ignore, stem=root / pred_path.stem)


def main(argv=None) -> None:
    logging.basicConfig(level=logging.INFO, format=cfg.LOGGING_FMT, datefmt=cfg.LOGGING_DATE_FMT)
    args = arg_parsing.parse_evaluation_args(argv)
    root = arg_parsing.root_path(args)
    labels_path = getattr(args, cfg.LABEL_DATA_ARG)
    settings_path = root / cfg.SETTINGS_DIR / cfg.PREDICTION_SETTINGS_FN
    pred_path = getattr(args, cfg.PREDICTION_ARG)
    if pred_path is not None:
        from types import SimpleNamespace
        from ..data import get_settings_data
        settings = get_settings_data(settings_path) if settings_path.is_file() else SimpleNamespace()
        _score_existing(root, pred_path, labels_path, settings)
        return
    from ..data import get_settings_data
    model_path, data_path = getattr(args, cfg.MODEL_PTH_ARG), getattr(args, cfg.PREDICT_DATA_ARG)
    settings = get_settings_data(settings_path)
    from ..model.operations.vol_seg_prediction_manager import VolSeg2DPredictionManager
    manager = VolSeg2DPredictionManager(str(model_path), data_path, settings)
    manager.evaluate_volume(labels_path, arg_parsing.prediction_output_path(root, data_path))


if __name__ == "__main__":
    main()
