"""Command lines of the commands (scripts/train_2d_model.py, scripts/predict_2d_model.py, scripts/evaluate_2d_model.py,
scripts/clean_2d_prediction.py, scripts/measure_2d_prediction.py, scripts/mesh_2d_prediction.py, scripts/thickness_2d_prediction.py);
the first two take the reference's arguments:

    train:    --data FILE [FILE ...] --labels FILE [FILE ...] [--data_dir DIR]
    predict:  MODEL FILE [--data_dir DIR]
    evaluate: MODEL FILE --labels LABELS [--data_dir DIR]   |   --prediction PRED --labels LABELS [--data_dir DIR]
    clean:    PRED [--data_dir DIR] [--output OUT]
    measure:  PRED [--data_dir DIR] [--output STEM]
    mesh:     PRED [--data_dir DIR] [--output STEM]
    thickness: PRED [--data_dir DIR] [--output STEM]

``--data_dir`` (default: the working directory) holds ``volseg-settings/`` and receives every output.  A volume or model file
with a suffix the engine does not read, or one that does not exist, is a usage error (argparse: exit status 2)."""
from __future__ import annotations

import argparse
import logging
import sys
from datetime import date
from pathlib import Path

from . import config as cfg


def existing_file_with_suffix(suffixes):
    """argparse ``type``: the path, refused unless its suffix is one of ``suffixes`` and the file exists."""
    allowed = sorted(suffixes)

    def convert(text: str) -> Path:
        path = Path(text)
        if path.suffix not in suffixes:
            raise argparse.ArgumentTypeError(f"wrong file type: {path} does not end with one of {allowed}")
        if not path.is_file():
            raise argparse.ArgumentTypeError(f"the file {path} does not appear to exist")
        return path
    return convert


def _add_data_dir(parser: argparse.ArgumentParser) -> None:
    parser.add_argument("--" + cfg.DATA_DIR_ARG, type=Path, default=None, metavar="DIR",
                        help=f'directory that holds "{cfg.SETTINGS_DIR}/" and receives the outputs (default: the working directory)')


def get_2d_training_parser() -> argparse.ArgumentParser:
    parser = argparse.ArgumentParser(description="Train a 2d segmentation model on 3d data volume(s) and their label volume(s).")
    parser.add_argument("--" + cfg.TRAIN_DATA_ARG, type=existing_file_with_suffix(cfg.TRAIN_DATA_EXT), nargs="+", required=True,
                        metavar="FILE", help="imaging data volume(s) to train on")
    parser.add_argument("--" + cfg.LABEL_DATA_ARG, type=existing_file_with_suffix(cfg.LABEL_DATA_EXT), nargs="+", required=True,
                        metavar="FILE", help="segmented label volume(s), one per data volume, in the same order")
    _add_data_dir(parser)
    return parser


def get_2d_prediction_parser() -> argparse.ArgumentParser:
    parser = argparse.ArgumentParser(description="Segment a 3d data volume with a trained 2d model.")
    parser.add_argument(cfg.MODEL_PTH_ARG, type=existing_file_with_suffix(cfg.MODEL_DATA_EXT), metavar="MODEL",
                        help="trained model file (.pytorch / .pth)")
    parser.add_argument(cfg.PREDICT_DATA_ARG, type=existing_file_with_suffix(cfg.PREDICT_DATA_EXT), metavar="FILE",
                        help="imaging data volume to segment")
    _add_data_dir(parser)
    return parser


def get_2d_evaluation_parser() -> argparse.ArgumentParser:
    """MODEL FILE --labels LABELS predicts and scores; --prediction PRED --labels LABELS scores an existing label volume."""
    parser = argparse.ArgumentParser(description="Score a segmentation against a labelled volume: predict with a trained 2d model "
                                                 "and score the result, or score an existing label volume (--prediction).")
    parser.add_argument(cfg.MODEL_PTH_ARG, type=existing_file_with_suffix(cfg.MODEL_DATA_EXT), metavar="MODEL", nargs="?", default=None,
                        help="trained model file (.pytorch / .pth)")
    parser.add_argument(cfg.PREDICT_DATA_ARG, type=existing_file_with_suffix(cfg.PREDICT_DATA_EXT), metavar="FILE", nargs="?", default=None,
                        help="imaging data volume to segment")
    parser.add_argument("--" + cfg.LABEL_DATA_ARG, type=existing_file_with_suffix(cfg.LABEL_DATA_EXT), required=True, metavar="LABELS",
                        help="labelled (ground-truth) volume to score against")
    parser.add_argument("--" + cfg.PREDICTION_ARG, type=existing_file_with_suffix(cfg.LABEL_DATA_EXT), default=None, metavar="PRED",
                        help="an existing predicted label volume to score instead of predicting (takes no MODEL / FILE)")
    _add_data_dir(parser)
    return parser


def parse_evaluation_args(argv=None) -> argparse.Namespace:
    """The evaluate command's arguments; exactly one of (MODEL and FILE) or --prediction, anything else is a usage error (exit 2)."""
    parser = get_2d_evaluation_parser()
    args = parser.parse_args(argv)
    model, data = getattr(args, cfg.MODEL_PTH_ARG), getattr(args, cfg.PREDICT_DATA_ARG)
    if getattr(args, cfg.PREDICTION_ARG) is not None:
        if model is not None or data is not None:
            parser.error("--prediction scores an existing label volume: give no MODEL or FILE with it")
    elif model is None or data is None:
        parser.error("give MODEL and FILE to predict and score, or --prediction PRED to score an existing label volume")
    return args


def _label_volume_parser(description: str, pred_help: str, metavar: str, output_help: str) -> argparse.ArgumentParser:
    """PRED [--data_dir DIR] [--output OUT | STEM]: the command line of the commands that work on an existing label volume"""
    parser = argparse.ArgumentParser(description=description)
    parser.add_argument(cfg.PREDICTION_ARG, type=existing_file_with_suffix(cfg.LABEL_DATA_EXT), metavar="PRED", help=pred_help)
    parser.add_argument("--output", type=Path, default=None, metavar=metavar, help=output_help)
    _add_data_dir(parser)
    return parser


def get_2d_cleaning_parser() -> argparse.ArgumentParser:
    """PRED [--data_dir DIR] [--output OUT]: clean an existing label volume with the postprocess_* keys of the predict settings."""
    return _label_volume_parser("Clean a predicted label volume: drop small connected components, keep the largest "
                                "component of a class, fill small enclosed holes (postprocess_* settings keys).",
                                "the label volume to clean", "OUT",
                                "where the cleaned volume goes (default: <stem of PRED>_cleaned.h5 under the data directory)")


def get_2d_measuring_parser() -> argparse.ArgumentParser:
    """PRED [--data_dir DIR] [--output STEM]: measure the objects of an existing label volume with the measure_* keys of the predict settings."""
    return _label_volume_parser("Measure the objects of a label volume: per connected component its voxels, centroid, "
                                "bounding box, surface, principal axes (measure_* settings keys).",
                                "the label volume to measure", "STEM",
                                "the files written are STEM_objects.csv and STEM_objects.json (default: <stem of PRED> under the data directory)")


def get_2d_meshing_parser() -> argparse.ArgumentParser:
    """PRED [--data_dir DIR] [--output STEM]: mesh the surfaces of an existing label volume with the mesh_* keys of the predict settings."""
    return _label_volume_parser("Export surface meshes of a label volume: per label value a closed surface net as binary "
                                "PLY or STL (mesh_* settings keys).",
                                "the label volume to mesh", "STEM",
                                "the files written are STEM_mesh_<value>.ply / .stl and STEM_meshes.json (default: <stem of PRED> under the data directory)")


def get_2d_thickness_parser() -> argparse.ArgumentParser:
    """PRED [--data_dir DIR] [--output STEM]: the local thickness of an existing label volume with the thickness_* keys of the predict settings."""
    return _label_volume_parser("Local thickness of a label volume: per label value, for every voxel the diameter of the largest "
                                "ball inside the material that contains it (thickness_* settings keys).",
                                "the label volume to measure", "STEM",
                                "the files written are STEM_thickness.csv, STEM_thickness.json and, with thickness_save_volume, STEM_thickness.h5 "
                                "(default: <stem of PRED> under the data directory)")


def parse_cleaning_args(argv=None) -> argparse.Namespace:
    """The clean command's arguments; an --output with a suffix the engine does not write is a usage error (exit 2)."""
    parser = get_2d_cleaning_parser()
    args = parser.parse_args(argv)
    if args.output is not None and args.output.suffix not in cfg.HDF5_SUFFIXES | cfg.NUMPY_SUFFIXES:
        parser.error(f"--output {args.output} does not end with one of {sorted(cfg.HDF5_SUFFIXES | cfg.NUMPY_SUFFIXES)}")
    return args


def _parse_stem_args(parser: argparse.ArgumentParser, argv) -> argparse.Namespace:
    args = parser.parse_args(argv)
    if args.output is not None and not args.output.resolve().parent.is_dir():
        parser.error(f"--output {args.output}: the directory {args.output.resolve().parent} does not exist")
    return args


def parse_measuring_args(argv=None) -> argparse.Namespace:
    """The measure command's arguments; an --output whose directory does not exist is a usage error (exit 2)."""
    return _parse_stem_args(get_2d_measuring_parser(), argv)


def parse_meshing_args(argv=None) -> argparse.Namespace:
    """The mesh command's arguments; an --output whose directory does not exist is a usage error (exit 2)."""
    return _parse_stem_args(get_2d_meshing_parser(), argv)


def parse_thickness_args(argv=None) -> argparse.Namespace:
    """The thickness command's arguments; an --output whose directory does not exist is a usage error (exit 2)."""
    return _parse_stem_args(get_2d_thickness_parser(), argv)


def open_label_volume(parse, argv) -> argparse.Namespace:
    """What the commands on an existing label volume do first: set up logging, parse with ``parse``, find the data directory, read the
    predict settings where the file exists (else none are set) and the volume.  Returns the arguments with ``settings``,
    ``settings_path``, ``pred_path``, ``pred``, ``chunking`` and ``stem`` - <stem of PRED> under the data directory - added."""
    logging.basicConfig(level=logging.INFO, format=cfg.LOGGING_FMT, datefmt=cfg.LOGGING_DATE_FMT)
    args = parse(argv)
    root = root_path(args)
    from types import SimpleNamespace
    from ..data import get_settings_data
    from . import base_data_utils as utils
    args.pred_path = getattr(args, cfg.PREDICTION_ARG)
    args.settings_path = root / cfg.SETTINGS_DIR / cfg.PREDICTION_SETTINGS_FN
    args.settings = get_settings_data(args.settings_path) if args.settings_path.is_file() else SimpleNamespace()
    args.pred, args.chunking = utils.get_numpy_from_path(args.pred_path, internal_path=getattr(args.settings, "data_hdf5_path", "/data"))
    args.stem = root / args.pred_path.stem
    return args


def root_path(args: argparse.Namespace) -> Path:
    given = getattr(args, cfg.DATA_DIR_ARG)
    return (Path.cwd() if given is None else Path(given)).resolve()


def check_volume_counts(data_vols, label_vols) -> None:
    if len(data_vols) != len(label_vols):
        logging.error("Number of data volumes and number of label volumes must be equal!")
        sys.exit(1)


def model_output_path(root: Path, model_type_name: str, model_output_fn: str, today: date | None = None) -> Path:
    """<date>_<type>_<model_output_fn>.pytorch under ``root``."""
    return Path(root) / f"{today or date.today()}_{model_type_name}_{model_output_fn}.pytorch"


def prediction_output_path(root: Path, data_vol_path: Path, today: date | None = None) -> Path:
    """<date>_<stem of the data file>_2d_model_vol_pred.h5 under ``root``."""
    return Path(root) / f"{today or date.today()}_{Path(data_vol_path).stem}_2d_model_vol_pred.h5"
