"""utilities/label_volume.py on the host: the shared rules of the label-volume analyses, and that the modules under utilities/ borrow
no private name from one another."""
import math
import re
from pathlib import Path

import numpy as np
import pytest

from volume_segmantics_amd.utilities import label_volume as lv


def test_zyx_pads_to_three_axes_and_refuses_the_rest():
    assert lv.zyx((7,)) == (1, 1, 7)
    assert lv.zyx((5, 7)) == (1, 5, 7)
    assert lv.zyx((3, 5, 7)) == (3, 5, 7)
    assert lv.zyx(np.zeros((2, 3), dtype=np.uint8).shape) == (1, 2, 3)
    for shape in ((), (0,), (3, 0, 2), (1, 2, 3, 4)):
        with pytest.raises(ValueError, match="one to three dimensions"):
            lv.zyx(shape)


def test_strict_conversion_refuses_what_does_not_fit():
    u8 = np.arange(6, dtype=np.uint8).reshape(2, 3)
    assert lv.strict_u8(u8) is u8                                     # as it came
    flags = lv.strict_u8(np.array([True, False, True]))
    assert flags.dtype == np.uint8 and flags.tolist() == [1, 0, 1]
    wide = lv.strict_u8(np.array([0, 255, 7], dtype=np.int64))
    assert wide.dtype == np.uint8 and wide.tolist() == [0, 255, 7]
    with pytest.raises(TypeError, match="integer label volume"):
        lv.strict_u8(np.zeros(3, dtype=np.float32))
    with pytest.raises(ValueError, match="do not fit uint8"):
        lv.strict_u8(np.array([0, 256], dtype=np.int32))
    with pytest.raises(ValueError, match="do not fit uint8"):
        lv.strict_u8(np.array([-1, 3], dtype=np.int16))


def test_lenient_conversion_marks_misfits_255():
    u8 = np.arange(6, dtype=np.uint8)
    assert lv.lenient_u8(u8) is u8
    assert lv.lenient_u8(np.array([True, False])).tolist() == [1, 0]
    out = lv.lenient_u8(np.array([0, 254, 255, 256, -1, 100000, 3], dtype=np.int64))
    assert out.dtype == np.uint8 and out.tolist() == [0, 254, 255, 255, 255, 255, 3]
    with pytest.raises(TypeError, match="integer label volume"):
        lv.lenient_u8(np.zeros(3, dtype=np.float64))


def test_voxel_size_is_one_positive_number_or_three():
    assert lv.voxel_size(2) == (2.0, 2.0, 2.0)
    assert lv.voxel_size([2.0, 1.0, 0.5]) == (2.0, 1.0, 0.5)
    for bad in ([1.0, 2.0], 0.0, [1.0, -1.0, 1.0], float("nan"), [1.0, float("inf"), 1.0]):
        with pytest.raises(ValueError, match="voxel size"):
            lv.voxel_size(bad)


def test_json_number_writes_nan_as_null_and_infinity_as_a_string():
    assert lv.json_number(float("nan")) is None
    assert lv.json_number(np.float64("inf")) == "inf" and lv.json_number(-math.inf) == "inf"
    value = lv.json_number(np.float32(0.25))
    assert type(value) is float and value == 0.25


def test_device_choice_is_none_for_the_host():
    assert lv.pick_device("cpu") is None
    assert lv.pick_device("cpu", np.zeros(3, dtype=np.uint8)) is None


def test_touch_mask_skips_axes_of_length_one():
    mask = lv.touch_mask((1, 3, 4))
    assert mask.shape == (1, 3, 4) and not mask[0, 1, 1:3].any() and int(mask.sum()) == 12 - 2
    assert lv.prepare(np.zeros((3, 4), dtype=np.uint8), "cpu", lambda zyx, resident: 0, "labels")[:3] == ((3, 4), (1, 3, 4), None)


def test_no_module_under_utilities_borrows_a_private_name_from_a_sibling():
    """a text search: ``from .<sibling> import _name`` and ``<alias>._name`` where ``<alias>`` is a sibling imported with ``from . import``"""
    folder = Path(lv.__file__).parent
    siblings = {p.stem for p in folder.glob("*.py")}
    assert {"label_volume", "evaluation", "surface_distance", "components", "measurements", "meshes"} <= siblings
    found = []
    for path in sorted(folder.glob("*.py")):
        text = path.read_text()
        aliases = set()
        for module, names in re.findall(r"^\s*from \.(\w*) import ([^\n]+)", text, flags=re.M):
            for item in names.replace("(", "").replace(")", "").split(","):
                parts = item.split()
                if not parts:
                    continue
                if module in siblings and parts[0].startswith("_"):
                    found.append(f"{path.name}: from .{module} import {parts[0]}")
                if module == "" and parts[0] in siblings:
                    aliases.add(parts[-1])                            # "name" or "name as alias"
        for alias in sorted(aliases):
            for name in re.findall(rf"\b{alias}\.(_(?!_)\w+)", text):
                found.append(f"{path.name}: {alias}.{name}")
    assert not found, found
    imports = re.findall(r"^\s*(?:from|import) [^\n]+", (folder / "label_volume.py").read_text(), flags=re.M)
    assert not [line for line in imports if re.search(r"evaluation|surface_distance|components|measurements|meshes", line)], imports
