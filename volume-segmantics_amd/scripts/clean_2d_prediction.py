"""model-clean-2d: repair a predicted label volume - drop small connected components, keep the largest component of a class, fill
small enclosed holes.

    python -m volume_segmantics_amd.scripts.clean_2d_prediction PRED.h5 [--data_dir DIR] [--output OUT.h5]

Reads ``DIR/volseg-settings/2d_model_predict_settings.yaml`` for the keys ``postprocess_min_object_size``, ``postprocess_keep_largest``,
``postprocess_fill_holes`` and ``postprocess_connectivity`` (utilities/components.py says what each does), cleans the label volume
``PRED`` - one this engine or the reference wrote - and writes ``<stem of PRED>_cleaned.h5`` under ``DIR`` (or ``OUT``) with
``<stem of PRED>_components.json`` and ``.csv`` beside it: per label value the components and voxels before, cleared and
kept, and the holes filled.  Runs the HIP kernels on a GPU and the host route, with the same integers, on a host without one.  With
no key set the volume is copied and the report says so."""
from __future__ import annotations

import logging

from ..utilities import arg_parsing


def main(argv=None) -> None:
    a = arg_parsing.open_label_volume(arg_parsing.parse_cleaning_args, argv)
    from ..utilities import base_data_utils as utils
    from ..utilities import components
    if not components.postprocess_settings(a.settings)["active"]:
        logging.warning(f"no postprocess_* key is set in {a.settings_path}: the volume is copied as it is")
    cleaned, report = components.postprocess_label_volume(a.pred, a.settings)
    logging.info("Components of the label volume:\n" + components.component_report_table(report))
    out_path = a.output if a.output is not None else a.stem.parent / f"{a.pred_path.stem}_cleaned.h5"
    utils.save_data_to_hdf5(cleaned.astype(a.pred.dtype, copy=False), out_path, chunking=a.chunking)
    components.write_component_report(out_path.parent / a.pred_path.stem, report)


if __name__ == "__main__":
    main()
