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


def main(argv=None) -> None:
    a = arg_parsing.open_label_volume(arg_parsing.parse_meshing_args, argv)
    from ..utilities import meshes
    m = meshes.mesh_label_volume(a.pred, a.settings)
    logging.info("Surface meshes of the label volume:\n" + meshes.mesh_summary_text(m["summary"]))
    meshes.write_meshes(a.output if a.output is not None else a.stem, m)


if __name__ == "__main__":
    main()
