"""model-thickness-2d: the local thickness of a label volume - per label value, for every voxel the diameter of the largest ball
that fits inside the material and contains the voxel.

    python -m volume_segmantics_amd.scripts.thickness_2d_prediction PRED.h5 [--data_dir DIR] [--output STEM]

Reads ``DIR/volseg-settings/2d_model_predict_settings.yaml`` for the keys ``thickness_values``, ``thickness_voxel_size``,
``thickness_save_volume`` and ``thickness_max_work`` (utilities/thickness.py says what each does), measures the label volume ``PRED`` - one
this engine or the reference wrote - and writes ``<stem of PRED>_thickness.csv`` and ``_thickness.json`` under ``DIR`` (or
``STEM_thickness.csv`` / ``.json``), with ``thickness_save_volume`` also ``_thickness.h5``, the float32 thicknesses.  Runs the HIP kernels
on a GPU and the host route, with the same integers, on a host without one - that route is for small volumes.  It measures whether
or not ``thickness_map`` is set: running the command is the request."""
from __future__ import annotations

import logging

from ..utilities import arg_parsing


def main(argv=None) -> None:
    a = arg_parsing.open_label_volume(arg_parsing.parse_thickness_args, argv)
    from ..utilities import base_data_utils as utils
    from ..utilities import thickness
    t = thickness.thickness_label_volume(a.pred, a.settings)
    logging.info("Local thickness of the label volume:\n" + thickness.thickness_summary_text(t))
    stem = a.output if a.output is not None else a.stem
    thickness.write_thickness(stem, t)
    if t["volume"] is not None:
        utils.save_data_to_hdf5(t["volume"], f"{stem}_thickness.h5", chunking=a.chunking)


if __name__ == "__main__":
    main()
