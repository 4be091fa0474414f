"""model-measure-2d: measure the objects of a label volume - per connected component its voxels, centroid, bounding box, face-count
surface, principal axes and whether it touches the boundary.

    python -m volume_segmantics_amd.scripts.measure_2d_prediction PRED.h5 [--data_dir DIR] [--output STEM]

Reads ``DIR/volseg-settings/2d_model_predict_settings.yaml`` for the keys ``measure_connectivity``, ``measure_min_voxels``,
``measure_background``, ``measure_voxel_size`` and ``measure_save_ids`` (utilities/measurements.py says what each does), measures the
label volume ``PRED`` - one this engine or the reference wrote - and writes ``<stem of PRED>_objects.csv`` and ``_objects.json`` under
``DIR`` (or ``STEM_objects.csv`` / ``.json``), with ``measure_save_ids`` also ``_object_ids.h5``.  Runs the HIP kernels on a GPU and the
host route, with the same integers, on a host without one.  It measures whether or not ``measure_objects`` is set: running the
command is the request.  With ``measure_separate: true`` (and ``measure_separate_values``, ``measure_separate_depth``,
``measure_separate_max_pairs``: utilities/separation.py) touching objects are taken apart first: the files describe the separated
objects and ``_object_contacts.csv`` / ``.json`` list the pairs that touch."""
from __future__ import annotations

import logging

from ..utilities import arg_parsing


def main(argv=None) -> None:
    a = arg_parsing.open_label_volume(arg_parsing.parse_measuring_args, argv)
    from ..utilities import base_data_utils as utils
    from ..utilities import measurements
    m = measurements.measure_label_volume(a.pred, a.settings)
    logging.info("Objects of the label volume:\n" + measurements.object_table_text(m["table"]) + measurements.separation_text(m))
    stem = a.output if a.output is not None else a.stem
    measurements.write_measurements(stem, m["raw"], m["table"], m["settings"], m.get("separation"))
    if m["ids"] is not None:
        utils.save_data_to_hdf5(m["ids"], f"{stem}_object_ids.h5", chunking=a.chunking)


if __name__ == "__main__":
    main()
