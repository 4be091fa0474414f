"""The volume feed's host side (data/volume_feed.py) and the two commands' argument handling, without a GPU.  The yardstick is
this repository's own PNG route: TrainingDataSlicer writes the slices, VolSeg2dDataset(augment="device") reads and fits them."""
import re
import subprocess
import sys
from datetime import date
from pathlib import Path

import numpy as np
import pytest

from volume_feed_cases import SIZE, VARIANTS, make_slicers, png_route_pairs, write_pngs

REPO = Path(__file__).resolve().parents[1]


@pytest.mark.parametrize("axes", ["All", "Y"])
def test_sample_table_follows_the_png_file_order(tmp_path, axes):
    from volume_segmantics_amd.data.datasets import natsort_key
    from volume_segmantics_amd.data.volume_feed import build_sample_table
    slicers = make_slicers("uint8_binary", shapes=((3, 12, 11), (13, 2, 5)), axes=axes)      # indices >= 10: "10" sorts after "2"
    data_dir, seg_dir = write_pngs(slicers, tmp_path)
    table = build_sample_table(slicers, SIZE)
    for directory, prefix in ((data_dir, "data"), (seg_dir, "seg")):
        files = sorted(directory.glob("*.png"), key=natsort_key)
        parsed = [re.fullmatch(rf"{prefix}(\d+)_([zyx])_stack_(\d+)\.png", f.name).groups() for f in files]
        assert [(int(k), a, int(i)) for k, a, i in parsed] == table.samples
    assert len(table) == (sum((3, 12, 11)) + sum((13, 2, 5)) if axes == "All" else 12 + 2)
    assert {a for _k, a, _i in table.samples} == ({"z", "y", "x"} if axes == "All" else {"y"})


@pytest.mark.parametrize("variant", VARIANTS)
def test_numpy_cut_equals_the_png_route_bit_for_bit(tmp_path, variant):
    from volume_segmantics_amd.data.volume_feed import BORDER_EDGE, build_sample_table, cut_numpy
    slicers = make_slicers(variant)
    want_images, want_masks = png_route_pairs(slicers, tmp_path)
    table = build_sample_table(make_slicers(variant), SIZE)      # fresh slicers: nothing the PNG route did is reused
    d = table.descriptors
    assert len(table) == len(want_images) == sum(sum(s.data_vol.shape) for s in slicers)
    # the cases do reach every branch: copies, up- and down-scaling, a pad wider than the slice, the edge border
    scaled = (d["nh"] != d["h"]) | (d["nw"] != d["w"])
    assert (~scaled).any() and (scaled & (d["nh"] > d["h"])).any() and (scaled & (d["nh"] < d["h"])).any()
    assert (d["top"] > d["nh"]).any() and (d["border"] == BORDER_EDGE).any() and (d["col_stride"] > 1).any()
    images, masks = cut_numpy(table.store.data, table.store.labels, d, SIZE)
    assert images.dtype == masks.dtype == np.uint8
    assert np.array_equal(images, want_images)
    assert np.array_equal(masks, want_masks)
    assert int(masks.max()) == max(s.num_seg_classes for s in slicers) - 1


def test_cpu_loader_yields_the_subset_in_sampler_order():
    import torch
    from volume_segmantics_amd.data.datasets import ShardedBatchSampler
    from volume_segmantics_amd.data.volume_feed import VolumeSliceLoader, build_sample_table, cut_numpy
    table = build_sample_table(make_slicers("three_classes", shapes=((7, 20, 32),)), SIZE)
    subset = [5, 0, 58, 5, 31, 17, 40]
    sampler = ShardedBatchSampler(len(subset), 3, shuffle=False, drop_last=False)
    loader = VolumeSliceLoader(table.subset(subset), sampler, "cpu")
    batches = list(loader)
    assert len(loader) == len(batches) == 3 and [b[0].shape[0] for b in batches] == [3, 3, 1]
    assert batches[0][0].shape == (3, 1, SIZE, SIZE) and batches[0][1].shape == (3, SIZE, SIZE) and batches[0][0].dtype == torch.uint8
    images, masks = cut_numpy(table.store.data, table.store.labels, table.descriptors[subset], SIZE)
    assert np.array_equal(torch.cat([b[0] for b in batches])[:, 0].numpy(), images)
    assert np.array_equal(torch.cat([b[1] for b in batches]).numpy(), masks)
    assert loader.max_label == 2
    loader.num_labels = 2
    with pytest.raises(RuntimeError, match="Class values must be smaller than num_classes."):
        next(iter(loader))
    empty_share = VolumeSliceLoader(table.subset([1]), ShardedBatchSampler(1, 2, rank=1, world=2, shuffle=False, drop_last=False), "cpu")
    assert list(empty_share) == [None]


def test_table_refuses_mismatched_volumes():
    from volume_segmantics_amd.data import TrainingDataSlicer
    from volume_segmantics_amd.data.volume_feed import build_sample_table
    from volume_feed_cases import settings
    slicer = TrainingDataSlicer(np.zeros((4, 5, 6), np.uint8), np.zeros((4, 5, 7), np.uint8), settings())
    with pytest.raises(ValueError, match="differ in shape"):
        build_sample_table([slicer], SIZE)
    big = TrainingDataSlicer(np.random.default_rng(0).random((2, 3, 4)).astype(np.float32) * 3, np.zeros((2, 3, 4), np.uint8), settings())
    with pytest.raises(ValueError, match="between -1 and 1"):      # img_as_ubyte's own error, as the PNG route raises it
        build_sample_table([big], SIZE)


# ---- the commands' arguments ---------------------------------------------------------------------------------------------------
def _touch(path):
    path.write_bytes(b"")
    return str(path)


def test_train_command_exits_1_on_unequal_numbers_of_volumes(tmp_path):
    """Through ``python -m`` in a fresh child: the entry point itself, before any settings file is read."""
    cmd = [sys.executable, "-m", "volume_segmantics_amd.scripts.train_2d_model", "--data", _touch(tmp_path / "a.h5"),
           _touch(tmp_path / "b.h5"), "--labels", _touch(tmp_path / "la.h5"), "--data_dir", str(tmp_path)]
    done = subprocess.run(cmd, cwd=REPO, capture_output=True, text=True, timeout=120)
    assert done.returncode == 1, done.stderr
    assert "must be equal" in done.stderr


def test_parsers_refuse_wrong_suffixes_and_missing_files(tmp_path, capsys):
    from volume_segmantics_amd.utilities.arg_parsing import get_2d_prediction_parser, get_2d_training_parser
    good, labels = _touch(tmp_path / "vol.tif"), _touch(tmp_path / "seg.npy")
    args = get_2d_training_parser().parse_args(["--data", good, "--labels", labels])
    assert args.data == [Path(good)] and args.labels == [Path(labels)] and args.data_dir is None
    for bad in (["--data", _touch(tmp_path / "vol.png"), "--labels", labels], ["--data", good, "--labels", _touch(tmp_path / "seg.txt")],
                ["--data", str(tmp_path / "absent.h5"), "--labels", labels]):
        with pytest.raises(SystemExit) as e:
            get_2d_training_parser().parse_args(bad)
        assert e.value.code == 2
    model = _touch(tmp_path / "m.pytorch")
    args = get_2d_prediction_parser().parse_args([model, good, "--data_dir", str(tmp_path)])
    assert args.model == Path(model) and args.data == Path(good) and args.data_dir == tmp_path
    for bad in ([_touch(tmp_path / "m.zip"), good], [model, _touch(tmp_path / "vol.jpg")]):
        with pytest.raises(SystemExit) as e:
            get_2d_prediction_parser().parse_args(bad)
        assert e.value.code == 2
    assert "wrong file type" in capsys.readouterr().err


def test_output_names_follow_the_reference_pattern(tmp_path):
    from volume_segmantics_amd.utilities.arg_parsing import model_output_path, prediction_output_path
    day = date(2024, 3, 9)
    assert model_output_path(tmp_path, "U_NET", "trained_2d_model", day) == tmp_path / "2024-03-09_U_NET_trained_2d_model.pytorch"
    assert prediction_output_path(tmp_path, Path("/x/vessels_DATA.h5"), day) == tmp_path / "2024-03-09_vessels_DATA_2d_model_vol_pred.h5"
    assert model_output_path(tmp_path, "FPN", "m").name == f"{date.today()}_FPN_m.pytorch"


# ---- does-not-fit: every rank takes the PNG route, or none does ------------------------------------------------------------------
def test_get_volume_training_loaders_gives_none_when_the_volumes_do_not_fit(monkeypatch):
    from volume_segmantics_amd.data import volume_feed
    from volume_feed_cases import settings
    slicers = make_slicers("uint8_binary", shapes=((7, 20, 32),))
    s = settings(batch_size=4, training_set_proportion=0.8, cuda_device=0)
    train, valid = volume_feed.get_volume_training_loaders(slicers, s, device="cpu")
    assert len(train.table) == int(59 * 0.8) and len(valid.table) == 59 - int(59 * 0.8)
    monkeypatch.setattr(volume_feed, "_fits_device_memory", lambda table, device: False)
    assert volume_feed.get_volume_training_loaders(slicers, s, device="cpu") is None


def test_from_volumes_falls_back_to_the_png_route(tmp_path, monkeypatch):
    from volume_segmantics_amd.data import get_settings_data, volume_feed
    from volume_segmantics_amd.data.datasets import natsort_key
    from volume_segmantics_amd.model.operations.vol_seg_2d_trainer import VolSeg2dTrainer
    monkeypatch.setattr(volume_feed, "_fits_device_memory", lambda table, device: False)
    s = get_settings_data(REPO / "volseg-settings" / "2d_model_train_settings.yaml")
    s.image_size, s.batch_size, s.augment, s.num_workers = SIZE, 4, "host", 0
    slicers = make_slicers("uint8_binary", shapes=((7, 20, 32), (3, 12, 11)))
    with pytest.raises(RuntimeError, match="no png_dirs"):
        VolSeg2dTrainer.from_volumes(slicers, 2, s)
    trainer = VolSeg2dTrainer.from_volumes(slicers, 2, s, png_dirs=(tmp_path / "data", tmp_path / "seg"))
    assert not isinstance(trainer.training_loader, volume_feed.VolumeSliceLoader)
    names = [f.name for f in sorted((tmp_path / "data").glob("*.png"), key=natsort_key)]
    assert len(names) == 59 + 26 == len(list((tmp_path / "seg").glob("*.png"))) and names[0] == "data0_x_stack_0.png"
    assert names[-1] == "data1_z_stack_2.png" and len(trainer.training_loader) == int(85 * 0.8) // 4
    slicers[-1].clean_up_slices()          # the slicers know the directories: the train command's clean-up removes them
    assert not (tmp_path / "data").exists() and not (tmp_path / "seg").exists()


def _agree_worker(rank, world, port, out_dir):
    import os
    sys.path.insert(0, str(REPO)); sys.path.insert(0, str(REPO / "tests"))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank),
                      VOLSEG_DIST_TIMEOUT_S="120")
    import torch
    torch.set_num_threads(2)
    from volume_feed_cases import make_slicers as make, settings
    from volume_segmantics_amd import dist as vdist
    from volume_segmantics_amd.data import volume_feed
    assert vdist.init_from_env("gloo")[:2] == (rank, world)
    s = settings(batch_size=2, training_set_proportion=0.8, cuda_device=0)
    slicers = make("uint8_binary", shapes=((3, 12, 11),))
    got = []
    for verdicts in ((True, True), (True, False), (False, True)):       # rank-local verdicts of (rank 0, rank 1)
        volume_feed._fits_device_memory = lambda table, device, v=verdicts[rank]: v
        loaders = volume_feed.get_volume_training_loaders(slicers, s, rank, world, device="cpu")
        got.append(loaders is not None)
        if loaders is not None:      # the ranks' shards of one global batch are disjoint halves of the same permutation
            first = next(iter(loaders[0].batch_sampler))
            assert len(first) == 2
    Path(out_dir, f"rank{rank}.txt").write_text(repr(got))
    vdist.barrier()


def test_ranks_agree_on_the_feed_by_one_all_reduced_minimum(tmp_path):
    import socket

    import torch.multiprocessing as mp
    for attempt in range(2):
        with socket.socket() as sock:
            sock.bind(("127.0.0.1", 0))
            port = sock.getsockname()[1]
        try:
            mp.spawn(_agree_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
            break
        except Exception as e:   # only the bind race is retried
            if attempt or not any(m in str(e) for m in ("Address already in use", "EADDRINUSE", "address already in use")):
                raise
    assert (tmp_path / "rank0.txt").read_text() == (tmp_path / "rank1.txt").read_text() == repr([True, False, False])
