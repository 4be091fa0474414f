"""model-mesh-2d: export surface meshes of a label volume - per label value a closed surface net as binary PLY or STL.

    python -m volume_segmantics_amd.scripts.mesh_2d_prediction PRED.h5 [--data_dir DIR] [--output STEM]

Reads ``DIR/volseg-settings/2d_model_predict_settings.yaml`` for the keys ``mesh_values``, ``mesh_style``, ``mesh_format``,
``mesh_triangulate`` and ``mesh_voxel_size`` (utilities/meshes.py says what each does), meshes the label volume ``PRED`` - one this
engine or the reference wrote - and writes ``<stem of PRED>_mesh_<value>.ply`` / ``.stl`` and ``_meshes.json`` under ``DIR`` (or
``STEM_mesh_<value>...`` / ``STEM_meshes.json``).  Runs the HIP kernels on a GPU and the host route, with the same bits, on a host
without one.  It meshes whether or not ``mesh_surfaces`` is set: running the command is the request."""
from __future__ import annotations

import logging

from ..utilities import arg_parsing
from ..utilities import config as cfg


def main(argv=None) -> None:
    logging.basicConfig(level=logging.INFO, format=cfg.LOGGING_FMT, datefmt=cfg.LOGGING_DATE_FMT)
    args = arg_parsing.parse_meshing_args(argv)
    root = arg_parsing.root_path(args)
    pred_path = getattr(args, cfg.PREDICTION_ARG)
    settings_path = root / cfg.SETTINGS_DIR / cfg.PREDICTION_SETTINGS_FN
    from types import SimpleNamespace
    from ..data import get_settings_data
    from ..utilities import base_data_utils as utils
    from ..utilities import meshes
    settings = get_settings_data(settings_path) if settings_path.is_file() else SimpleNamespace()
    pred, _ = utils.get_numpy_from_path(pred_path, internal_path=getattr(settings, "data_hdf5_path", "/data"))
    m = meshes.mesh_label_volume(pred, settings)
    logging.info("Surface meshes of the label volume:\n" + meshes.mesh_summary_text(m["summary"]))
    stem = args.output if args.output is not None else root / pred_path.stem
    meshes.write_meshes(stem, m)


if __name__ == "__main__":
    main()
