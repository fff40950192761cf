"""World-size-2 and -3 gloo tests of batched draws for sharded scenes on the CPU: renderer_amd.sharded.BatchExchange over the
stand-in (tests/cpu_batch_pipeline.py) — shard chunks, one all-gather, the merge — equals the unsharded restatement
(lod_restatement.batch_draws_lods of the whole scene), with and without tighten(); a tightened chunk that overflows when the
camera moves is repaired once, on every rank, with nothing lost."""
import os
import sys
import tempfile

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
BASE = 77   # the global first_instance_base


def _setup(rank, world, init_file, n_global):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, HERE)
    from cpu_batch_pipeline import BatchOraclePipeline
    from renderer_amd import scene
    from renderer_amd.pipeline import make_frame
    from renderer_amd.sharded import BatchExchange, shard_range

    dist.init_process_group("gloo", init_method=f"file://{init_file}", rank=rank, world_size=world)
    full = scene.make_scene(3, n=n_global)
    lo, hi = shard_range(n_global, world, rank)
    shard = scene.make_scene(3, n=hi - lo, first=lo)
    assert np.array_equal(shard["pos"], full["pos"][lo:hi])
    pipe = BatchOraclePipeline(shard)
    ex = BatchExchange(pipe, hi - lo, world, rank, torch.device("cpu"), pipe.n_buckets, dist=dist, torch=torch)

    def frames(planes, cam):
        return make_frame(planes, cam, first_instance_base=BASE + lo)

    return full, ex, frames, hi - lo


def _run(ex, frame, n_local):
    """The shard's frame (its bitmap), then the exchange over that bitmap."""
    from lod_restatement import DISTANCE
    from renderer_amd.pipeline import make_lod_policy

    bitmap = torch.zeros((n_local + 31) // 32 + 1, dtype=torch.int32)
    ex.pipe.run_device(frame, visible_bitmap=bitmap.data_ptr())
    ex.step(frame, bitmap.data_ptr(), make_lod_policy(DISTANCE, SWITCH))
    return bitmap


SWITCH = (9.0, 36.0, 100.0, 400.0, 1600.0)


def _want(full, planes, cam):
    import oracle
    from lod_restatement import DISTANCE, batch_draws_lods

    vis = oracle.run(full["pos"], full["rot"], full["scale"], full["mesh_id"], full["meshes"], planes, cam)["visible_bitmap"]
    return batch_draws_lods(full["pos"], full["scale"], full["mesh_id"], full["meshes"], cam, vis, DISTANCE, SWITCH, first_instance_base=BASE)


def _check(ex, want, what):
    cmds, count, ids, members = ex.merged_batches()
    assert (count, members) == (want["count"], want["members"]), (what, count, members, want["count"], want["members"])
    assert cmds.tobytes() == want["cmds"].tobytes(), what
    assert ids.tobytes() == want["ids"].tobytes(), what


def _worker(rank, world, init_file, n_global, tighten, out_dir):
    try:
        full, ex, frames, n_local = _setup(rank, world, init_file, n_global)
        want = _want(full, full["planes"], full["cam_pos"])
        frame = frames(full["planes"], full["cam_pos"])
        _run(ex, frame, n_local)
        _check(ex, want, "full capacity")
        assert want["members"] > 0 or n_global < 10
        if tighten:
            cap = ex.tighten()
            assert cap <= max(ex.n_max, 256) and ex.stride % 256 == 0
            _run(ex, frame, n_local)
            _check(ex, want, "tightened")
            assert ex.retries == 0
        open(os.path.join(out_dir, f"ok{rank}"), "w").write("ok")
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world,n_global,tighten", [(2, 20_000, False), (2, 4_097, True), (3, 1_000, True), (3, 1_000, False), (2, 1, False),
                                                   (3, 2, True)])
def test_batch_exchange_matches_the_unsharded_restatement(world, n_global, tighten):
    with tempfile.TemporaryDirectory() as d:
        mp.spawn(_worker, args=(world, os.path.join(d, "init"), n_global, tighten, d), nprocs=world, join=True)
        for r in range(world):
            assert os.path.exists(os.path.join(d, f"ok{r}"))


def _worker_overflow(rank, world, init_file, n_global, out_dir):
    try:
        from renderer_amd._lib import MipError
        from test_sharded_gloo import _camera_b

        full, ex, frames, n_local = _setup(rank, world, init_file, n_global)
        planes_b, cam_b = _camera_b()
        frame_a, frame_b = frames(full["planes"], full["cam_pos"]), frames(planes_b, cam_b)
        want_a, want_b = _want(full, full["planes"], full["cam_pos"]), _want(full, planes_b, cam_b)
        assert want_b["members"] > 1.2 * want_a["members"]
        _run(ex, frame_a, n_local)
        _check(ex, want_a, "A, full capacity")
        cap = ex.tighten()
        assert cap < n_local
        _run(ex, frame_a, n_local)
        _check(ex, want_a, "A, tightened")
        assert ex.retries == 0
        _run(ex, frame_b, n_local)            # the camera moved between tighten() and this frame
        _check(ex, want_b, "B, overflow repaired")
        assert ex.retries == 1 and ex.capacity == ex.n_max
        _run(ex, frame_a, n_local)
        _check(ex, want_a, "A again")
        assert ex.retries == 1
        # one rank's wait reports ANOTHER error for the overflowing frame: it still takes part in the collective repair, decided
        # from the gathered `members` words, and reports its own error afterwards
        ex.tighten()
        _run(ex, frame_a, n_local)
        _check(ex, want_a, "A, tightened again")
        if rank == world - 1:
            ex.pipe.other_error_once = -5
        _run(ex, frame_b, n_local)
        if rank == world - 1:
            with pytest.raises(MipError) as e:
                ex.complete()
            assert e.value.code == -5
        else:
            assert ex.complete() is True
        assert ex.retries == 2 and ex.capacity == ex.n_max
        _check(ex, want_b, "B, repaired by every rank although one had a different error")
        open(os.path.join(out_dir, f"ok{rank}"), "w").write("ok")
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world,n_global", [(2, 6_000), (3, 5_001)])
def test_overflow_of_a_tightened_batch_chunk_is_repaired_not_lost(world, n_global):
    with tempfile.TemporaryDirectory() as d:
        mp.spawn(_worker_overflow, args=(world, os.path.join(d, "init"), n_global, d), nprocs=world, join=True)
        for r in range(world):
            assert os.path.exists(os.path.join(d, f"ok{r}"))
