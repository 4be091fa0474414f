"""VolSeg2DPredictionManager - volume in, label volume out / to disk
(reference: volume_segmantics/model/operations/vol_seg_prediction_manager.py:12-100)."""
import logging
from pathlib import Path
from types import SimpleNamespace
from typing import Callable, NamedTuple, Union

import numpy as np

from ...data.base_data_manager import BaseDataManager
from ...utilities import base_data_utils as utils
from ...utilities import components, measurements, meshes, thickness
from .vol_seg_2d_predictor import VolSeg2dPredictor


class LabelStep(NamedTuple):
    """One optional step on the merged label volume.  The functions of the utilities modules are looked up when a step runs."""
    name: str
    asked: Callable       # settings -> whether the settings ask for the step
    refusal: str          # why ``one_hot: True`` cannot have it, and what to unset
    run: Callable         # (volume, settings, device) -> (the volume to go on with, what to remember), or None: nothing to do after all
    log: Callable         # what is remembered -> the text for the log
    remember: str         # the manager's attribute that keeps it
    write: Callable       # (stem, what is remembered, save(array, path)) -> the files beside the label volume


def _clean(volume, settings, device):
    if not components.postprocess_settings(settings)["active"]:
        return None
    cleaned, report = components.postprocess_label_volume(volume, settings, device=device)
    return cleaned, {"raw": volume, "report": report}


def _write_measurements(stem, m, save):
    measurements.write_measurements(stem, m["raw"], m["table"], m["settings"], m.get("separation"))
    if m["ids"] is not None:
        save(m["ids"], f"{stem}_object_ids.h5")


def _write_thickness(stem, t, save):
    thickness.write_thickness(stem, t)
    if t["volume"] is not None:
        save(t["volume"], f"{stem}_thickness.h5")


# in the order they run: the measurements, the meshes and the thickness are those of the volume that is saved, after any cleanup
LABEL_STEPS = (
    LabelStep("clean", lambda s: any(getattr(s, key, None) for key in ("postprocess_min_object_size", "postprocess_keep_largest", "postprocess_fill_holes")),
              "there are no components to clean (unset the postprocess_* keys or set one_hot: False)", _clean,
              lambda kept: "Components of the merged label volume:\n" + components.component_report_table(kept["report"]),
              "last_postprocess", lambda stem, kept, save: components.write_component_report(stem, kept["report"])),
    LabelStep("measure", lambda s: bool(getattr(s, "measure_objects", False)),
              "there are no objects to measure (unset measure_objects or set one_hot: False)",
              lambda volume, s, device: (volume, measurements.measure_label_volume(volume, s, device=device)),
              lambda m: "Objects of the label volume:\n" + measurements.object_table_text(m["table"]) + measurements.separation_text(m),
              "last_measurements", _write_measurements),
    LabelStep("mesh", lambda s: bool(getattr(s, "mesh_surfaces", False)),
              "there is no surface to mesh (unset mesh_surfaces or set one_hot: False)",
              lambda volume, s, device: (volume, meshes.mesh_label_volume(volume, s, device=device)),
              lambda m: "Surface meshes of the label volume:\n" + meshes.mesh_summary_text(m["summary"]),
              "last_meshes", lambda stem, m, save: meshes.write_meshes(stem, m)),
    LabelStep("thickness", lambda s: bool(getattr(s, "thickness_map", False)),
              "there is no material to measure the thickness of (unset thickness_map or set one_hot: False)",
              lambda volume, s, device: (volume, thickness.thickness_label_volume(volume, s, device=device)),
              lambda t: "Local thickness of the label volume:\n" + thickness.thickness_summary_text(t),
              "last_thickness", _write_thickness),
)


class VolSeg2DPredictionManager(BaseDataManager):
    def __init__(self, model_file_path: str, data_vol: Union[str, np.ndarray], settings: SimpleNamespace) -> None:
        super().__init__(data_vol, settings)
        self.predictor = VolSeg2dPredictor(model_file_path, settings)
        self.settings = settings

    def get_label_codes(self) -> dict:
        return self.predictor.label_codes

    def predict_volume_to_path(self, output_path: Union[Path, None], quality: Union[utils.Quality, None] = None) -> np.ndarray:
        """LOW = one axis, MEDIUM = 3 axes, HIGH = 3 axes x 4 rotations, merged by maximum probability;
        ``one_hot`` returns per-class vote counts instead (:43-89).  With one of the optional settings keys ``postprocess_min_object_size``,
        ``postprocess_keep_largest`` or ``postprocess_fill_holes`` set, the merged label volume is cleaned (utilities/components.py, connected
        components under ``postprocess_connectivity``) before it is saved and returned: ``last_postprocess`` then keeps the raw volume and
        the report, and ``<stem>_components.json`` / ``.csv`` are written beside the label volume.  The probabilities stay as predicted.
        With ``measure_objects: true`` the volume about to be saved - after any cleanup - is measured (utilities/measurements.py: one row
        per connected component under ``measure_connectivity``, at least ``measure_min_voxels`` voxels, the background with
        ``measure_background``, physical units from ``measure_voxel_size``): the summary is logged, ``last_measurements`` keeps the raw
        integers and the table, and ``<stem>_objects.csv`` / ``.json`` - with ``measure_save_ids`` also ``<stem>_object_ids.h5`` - are
        written beside the label volume.  With ``measure_separate: true`` as well the rows, the ids and the files describe the objects a
        distance-map watershed takes apart (utilities/separation.py: ``measure_separate_values``, ``measure_separate_depth``,
        ``measure_separate_max_pairs``), ``last_measurements["separation"]`` keeps the report and the contacts, and
        ``<stem>_object_contacts.csv`` / ``.json`` list the pairs of touching objects.
        With ``mesh_surfaces: true`` the same volume is meshed (utilities/meshes.py: per value of ``mesh_values`` a closed surface net in
        ``mesh_style``, physical units from ``mesh_voxel_size``): the summary is logged, ``last_meshes`` keeps the arrays and the figures,
        and ``<stem>_mesh_<value>.ply`` / ``.stl`` (``mesh_format``, ``mesh_triangulate``) and ``<stem>_meshes.json`` are written beside the
        label volume.
        With ``thickness_map: true`` the same volume gets its local thickness (utilities/thickness.py: per value of ``thickness_values`` the
        diameter of the largest ball inside the material that contains the voxel, physical units from ``thickness_voxel_size``, the
        work bounded by ``thickness_max_work``): the per-value figures are logged, ``last_thickness`` keeps the squared map, the histograms
        and the figures, and ``<stem>_thickness.json`` / ``.csv`` - with ``thickness_save_volume`` also ``<stem>_thickness.h5``, the float32
        thicknesses - are written beside the label volume.
        ``voxel_spacing: [sz, sy, sx]`` states the grid for all of them (utilities/label_volume.py ``voxel_grid``): the default of
        ``measure_voxel_size`` and ``mesh_voxel_size``, the weighted distance map of ``measure_separate`` and of the thickness, whose
        files then carry ``voxel_spacing``, ``weights`` and ``unit``; it is an error beside ``thickness_voxel_size``."""
        one_hot = self.settings.one_hot
        steps = [step for step in LABEL_STEPS if step.asked(self.settings)]
        if one_hot and steps:
            raise ValueError("one_hot: True predicts per-class vote counts, not a label volume: " + steps[0].refusal)
        for step in LABEL_STEPS:
            setattr(self, step.remember, None)
        axis = utils.get_prediction_axis(self.settings)
        if quality is None:
            quality = utils.get_prediction_quality(self.settings)
        p, probs = self.predictor, None
        if quality == utils.Quality.LOW:
            if one_hot:
                prediction = p._predict_single_axis_to_one_hot(self.data_vol, axis=axis)
            else:
                prediction, probs = p._predict_single_axis(self.data_vol, axis=axis)
        elif quality == utils.Quality.MEDIUM:
            if one_hot:
                prediction = p._predict_3_ways_one_hot(self.data_vol)
            else:
                prediction, probs = p._predict_3_ways_max_probs(self.data_vol)
        elif quality == utils.Quality.HIGH:
            if one_hot:
                prediction = p._predict_12_ways_one_hot(self.data_vol)
            else:
                prediction, probs = p._predict_12_ways_max_probs(self.data_vol)
        else:
            raise ValueError(f"unknown quality {quality}")
        done = []
        for step in steps:
            # every rank that holds the merged volume works on it: exact integers and a fixed order of vertices and quads, so the ranks agree
            result = step.run(prediction, self.settings, f"cuda:{p.model_device_num}") if prediction is not None else None
            if result is not None:
                prediction, kept = result
                setattr(self, step.remember, kept)
                logging.info(step.log(kept))
                done.append((step, kept))
        if output_path is not None:
            output_path = Path(output_path)
            stem = output_path.parent / output_path.stem
            save = lambda data, path: utils.save_data_to_hdf5(data, path, chunking=self.input_data_chunking)      # noqa: E731
            save(prediction, output_path)
            if done:
                from ... import dist as vdist
                if vdist.world()[0] == 0:
                    for step, kept in done:
                        step.write(stem, kept, save)
            if probs is not None and self.settings.output_probs:
                # the reference hard-codes the name: "<stem>_probs.h5" whatever the label file's suffix (:94-98)
                save(probs, f"{stem}_probs.h5")
        return prediction

    def evaluate_volume(self, label_vol: Union[Path, str, np.ndarray], output_path: Union[Path, None] = None,
                        quality: Union[utils.Quality, None] = None, prediction: Union[np.ndarray, None] = None):
        """Score the segmentation of the data volume against the labelled volume ``label_vol`` (a path or an array): per-class
        Dice / IoU / precision / recall, voxel accuracy and the confusion matrix (utilities/evaluation.py).  Predicts through
        ``predict_volume_to_path`` unless ``prediction`` is given.  With ``output_path`` the label volume is written as usual and
        beside it ``<stem>_scores.csv``, ``<stem>_scores.json`` and, with the settings key ``evaluation_per_slice: true``,
        ``<stem>_scores_per_slice.csv``.  Class ``i`` is the ``i``-th ground-truth value in ascending order, from the checkpoint's
        label codes where they record the values (evaluation.truth_label_values); ``evaluation_ignore_label`` sets voxels aside.
        Returns the scores; ``last_evaluation`` keeps the prediction, the dropped counts and the per-slice Dice.  With the settings key
        ``evaluation_surface_distances: true`` the surface distances (utilities/surface_distance.py: Hausdorff, its 95th percentile,
        average symmetric surface distance, surface Dice at ``evaluation_surface_tolerance``, distances in ``evaluation_voxel_size``, or exact on the anisotropic grid of ``voxel_spacing``) are
        computed as well, logged, written to ``<stem>_surface_scores.csv`` / ``.json`` and kept in ``last_evaluation["surface_scores"]``.
        With ``evaluation_object_scores: true`` the object-level scores (utilities/object_scores.py: true and predicted connected
        components under ``evaluation_object_connectivity`` matched at ``evaluation_object_iou``; precision, recall, F1, panoptic quality,
        splits, merges, variation of information, adapted Rand error) are computed too, logged, written to ``<stem>_object_scores.csv``
        / ``.json`` and ``<stem>_object_matches.csv`` and kept in ``last_evaluation["object_scores"]``."""
        from ... import dist as vdist
        from ...utilities import evaluation as ev

        if self.settings.one_hot:
            raise ValueError("one_hot: True predicts per-class vote counts, not a label volume: there is nothing to score "
                             "(set one_hot: False to evaluate)")
        if isinstance(label_vol, (str, Path)):
            truth, _ = utils.get_numpy_from_path(Path(label_vol), internal_path=getattr(self.settings, "seg_hdf5_path", self.settings.data_hdf5_path))
        elif isinstance(label_vol, np.ndarray):
            truth = label_vol
        else:
            raise TypeError("label_vol must be a path or a numpy array")
        expected = tuple(self.data_vol.shape if prediction is None else prediction.shape)
        if expected != tuple(truth.shape):
            why = " (downsample: True halves the data volume before it is predicted: the labels must be of that size)" if self.downsample else ""
            raise ValueError(f"the prediction has shape {expected} but the label volume has shape {tuple(truth.shape)}{why}")
        rank0 = vdist.world()[0] == 0       # under torch.distributed every rank that holds the merged volume scores it; rank 0 writes
        if prediction is None:
            prediction = self.predict_volume_to_path(output_path if rank0 else None, quality)
        if prediction is None:        # a rank that does not hold the merged volume (predictor.result_ranks = "rank0")
            return None
        classes = int(self.predictor.num_labels)
        ignore = getattr(self.settings, "evaluation_ignore_label", None)
        per_slice = bool(getattr(self.settings, "evaluation_per_slice", False))
        values = ev.truth_label_values(self.get_label_codes(), truth, classes, ignore_label=ignore)
        device = f"cuda:{self.predictor.model_device_num}"
        scores, dropped, slab_dice = ev.evaluate_label_volumes(prediction, truth, classes, label_values=values, ignore_label=ignore,
                                                               per_slice=per_slice, device=device)
        self.last_evaluation = {"prediction": prediction, "dropped": dropped, "per_slice_dice": slab_dice, "label_values": values}
        logging.info("Scores against the label volume:\n" + ev.score_table(scores, values))
        if output_path is not None and rank0:
            output_path = Path(output_path)
            ev.write_scores(output_path.parent / output_path.stem, scores, dropped, values, slab_dice)
        from ...utilities import surface_distance as sd
        if sd.surface_settings(self.settings)[0]:
            stem = output_path.parent / output_path.stem if output_path is not None and rank0 else None
            self.last_evaluation["surface_scores"] = sd.evaluate_surface_distances(
                prediction, truth, classes, self.settings, label_values=values, ignore_label=ignore, device=device, stem=stem)[0]
        from ...utilities import object_scores as obs
        if obs.object_scores_asked(self.settings):
            stem = output_path.parent / output_path.stem if output_path is not None and rank0 else None
            self.last_evaluation["object_scores"] = obs.evaluate_objects(
                prediction, truth, classes, self.settings, label_values=values, ignore_label=ignore, device=device, stem=stem)[0]
        return scores
