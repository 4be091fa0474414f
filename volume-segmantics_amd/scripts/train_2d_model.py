"""model-train-2d: from data and label volume files to a trained model.

    python -m volume_segmantics_amd.scripts.train_2d_model --data DATA.h5 [...] --labels LABELS.h5 [...] [--data_dir DIR]

Reads ``DIR/volseg-settings/2d_model_train_settings.yaml``; writes ``DIR/<date>_<type>_<model_output_fn>.pytorch`` with its loss
figure, statistics CSV and prediction figure.  The optional settings key ``slice_feed`` picks how the slices reach the trainer:

    volume   (default with a GPU and device-side augmentation) the volumes are uploaded once and every batch is cut out of them
             on the device (data/volume_feed.py) - no PNG file is written
    png      the on-disk route: every slice of every axis is written as a PNG under DIR/<data_im_dirname> and
             DIR/<seg_im_out_dirname>, trained from, and removed again; also the default when ``resident_feed: false`` asks for the
             per-epoch DataLoader (an explicit ``slice_feed`` wins over ``resident_feed``)"""
from __future__ import annotations

import logging
import sys

from .. import dist as vdist
from ..data import TrainingDataSlicer, get_settings_data
from ..data.slicers import check_ignore_label_occurs
from ..data.volume_feed import volume_feed_applies
from ..utilities import arg_parsing
from ..utilities import base_data_utils as utils
from ..utilities import config as cfg


def main(argv=None) -> None:
    logging.basicConfig(level=logging.INFO, format=cfg.LOGGING_FMT, datefmt=cfg.LOGGING_DATE_FMT)
    args = arg_parsing.get_2d_training_parser().parse_args(argv)
    data_vols, label_vols = getattr(args, cfg.TRAIN_DATA_ARG), getattr(args, cfg.LABEL_DATA_ARG)
    arg_parsing.check_volume_counts(data_vols, label_vols)
    root = arg_parsing.root_path(args)
    settings = get_settings_data(root / cfg.SETTINGS_DIR / cfg.TRAIN_SETTINGS_FN)
    feed = getattr(settings, "slice_feed", None)
    if feed is None:      # an explicit `resident_feed: false` asks for the per-epoch DataLoader over PNG files: that is the png route
        wants_loader = getattr(settings, "resident_feed", None) is False
        feed = "volume" if volume_feed_applies(settings) and not wants_loader else "png"
    if feed not in ("volume", "png"):
        logging.error(f"slice_feed: {feed} is not valid. Options are ['volume', 'png'].")
        sys.exit(1)
    if feed == "volume" and not volume_feed_applies(settings):
        logging.error("slice_feed: volume needs a GPU and device-side augmentation (image_size a multiple of 8, augment not 'host').")
        sys.exit(1)
    from ..model.operations.vol_seg_2d_trainer import VolSeg2dTrainer, resolve_balanced_class_weights
    vdist.init_from_env()
    rank, _world = vdist.world()
    data_dir, seg_dir = root / settings.data_im_dirname, root / settings.seg_im_out_dirname
    slicers = [TrainingDataSlicer(d, l, settings) for d, l in zip(data_vols, label_vols)]
    check_ignore_label_occurs(slicers)
    widest = max(slicers, key=lambda s: s.num_seg_classes)      # (the first of equals, as the reference's loop keeps it)
    max_label_no, label_codes = widest.num_seg_classes, widest.codes
    settings = resolve_balanced_class_weights(settings, slicers, max_label_no)      # `loss_class_weights: balanced` -> the list
    if feed == "volume":
        trainer = VolSeg2dTrainer.from_volumes(slicers, max_label_no, settings, png_dirs=(data_dir, seg_dir))
    else:
        if rank == 0:
            for count, slicer in enumerate(slicers):
                slicer.output_data_slices(data_dir, f"data{count}")
                slicer.output_label_slices(seg_dir, f"seg{count}")
        vdist.barrier()
        trainer = VolSeg2dTrainer(data_dir, seg_dir, max_label_no, settings)
    logging.info(f"Label codes: {label_codes}")
    model_out = arg_parsing.model_output_path(root, utils.get_model_type(settings).name, settings.model_output_fn)
    frozen, unfrozen = int(settings.num_cyc_frozen), int(settings.num_cyc_unfrozen)
    if frozen > 0:
        trainer.train_model(model_out, frozen, settings.patience, create=True, frozen=True)
    if unfrozen > 0:
        trainer.train_model(model_out, unfrozen, settings.patience, create=frozen == 0, frozen=False)
    if rank == 0:
        trainer.output_loss_fig(model_out)
        trainer.output_prediction_figure(model_out)
    vdist.barrier()
    if rank == 0:
        slicers[-1].clean_up_slices()       # removes the slice directories when they were written (all slicers share them)


if __name__ == "__main__":
    main()
