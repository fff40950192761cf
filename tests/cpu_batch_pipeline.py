"""TEST-ONLY: cpu_pipeline.OraclePipeline extended with the batched-draws exchange — batch_draws_shard, merge_batches and the
deferred error in wait() — from the numpy restatements (lod_restatement.py, batch_merge_restatement.py), so that
renderer_amd.sharded.BatchExchange runs under gloo without a GPU. "Device pointers" are addresses of CPU torch tensors.
Never imported by the product."""
import numpy as np

import batch_merge_restatement as bm
from cpu_pipeline import OraclePipeline, _view
from renderer_amd._lib import MIP_OUT_ASYNC, MipError  # noqa: F401


class BatchOraclePipeline(OraclePipeline):
    def __init__(self, scene):
        super().__init__(scene)
        self.n_buckets = int(scene["meshes"]["n_lods"].sum())
        self._batch_error = None

    def batch_draws_shard(self, frame, visible_bitmap_ptr, policy, chunk_ptr, ids_capacity, async_=False):
        s = self.s
        if ids_capacity < self.n:
            raise MipError(-1, "ids_capacity below the resident instances")
        bitmap = _view(visible_bitmap_ptr, ((self.n + 31) // 32) * 4, np.uint32) if self.n else np.zeros(0, np.uint32)
        r = bm.lr.batch_draws_lods(s["pos"], s["scale"], s["mesh_id"], s["meshes"], np.array(frame.cam_pos[:], np.float32), bitmap,
                                   int(policy.mode), tuple(policy.switch_sq), first_instance_base=frame.first_instance_base)
        base, b = bm.lr.lod_bases(s["meshes"])
        inst = r["order"]
        counts = np.bincount(base[s["mesh_id"].astype(np.int64)[inst]] + r["lod"][inst], minlength=b).astype(np.uint32)
        off = bm.ids_offset_words(b)
        head = _view(chunk_ptr, off * 4, np.uint32)      # the header, the counts, the pad: written whole
        head[:4] = (r["members"], b, 0, 0)
        head[4:4 + b] = counts
        head[4 + b:] = 0
        if r["members"]:                                 # ids at or behind `members` are not touched
            _view(chunk_ptr + off * 4, r["members"] * 4, np.uint32)[:] = r["ids"]

    def merge_batches(self, chunks_ptr, n_chunks, chunk_stride_bytes, chunk_capacity, *, batch_cmds, batch_count, instance_ids,
                      instance_count=0, async_=False):
        b = self.n_buckets
        words = bm.chunk_bytes(b, chunk_capacity) // 4
        assert chunk_stride_bytes % 16 == 0 and chunk_stride_bytes >= words * 4
        chunks = [_view(chunks_ptr + k * chunk_stride_bytes, words * 4, np.uint32) for k in range(n_chunks)]
        status, out = bm.merge(chunks, chunk_capacity, self.s["meshes"])
        _view(batch_count, 4, np.uint32)[0] = out["batch_count"]
        if instance_count:
            _view(instance_count, 4, np.uint32)[0] = out["instance_count"]
        if status == bm.OK:
            if out["batch_count"]:
                _view(batch_cmds, out["batch_count"] * 20, np.uint32)[:] = out["cmds_words"][:out["batch_count"]].reshape(-1)
            if out["instance_count"]:
                _view(instance_ids, out["instance_count"] * 4, np.uint32)[:] = out["ids"][:out["instance_count"]]
        else:   # deferred, as the library defers it to mip_wait for an asynchronous call
            self._batch_error = MipError(status, "a batch chunk is corrupt" if status == bm.ERR_DEVICE else
                                         "a shard's batch chunk holds more members than the exchanged chunk_capacity")
            if not async_:
                self.wait()

    def wait(self):
        """As mip_wait: the deferred status of an asynchronous merge_batches — or, when the test has planted one
        (`other_error_once`), ANOTHER code that mip_wait ranks above it."""
        err, self._batch_error = self._batch_error, None
        if err is not None:
            code = getattr(self, "other_error_once", None)
            if code is not None:
                self.other_error_once = None
                raise MipError(code, "a local error that outranks the overflow in mip_wait")
            raise err
        super().wait()
