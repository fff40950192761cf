"""The decompositions of the per-triangle stage (row f-1) and how a test forces one: shared by tests/test_gpu_triangles.py and
tests/test_gpu_triangle_edges.py."""

MODES = ["ranges", "ranges_ticketed", "ranges_or_sorted_waves", "sorted_waves", "ranges_of_a_large_frame", "recompact_three_launches",
         "wave", "wave_only", "tickets", "tickets_x4", "block256", "block512", "block1024", "parts"]


def force_variant(monkeypatch, mode):
    """Forces one decomposition of the stage (tuning variables, read by mip_create and at launch)."""
    if mode == "ranges":
        pass                                                     # the default at this size: one range per wave
    elif mode == "ranges_ticketed":
        monkeypatch.setenv("MIP_TUNE_TRI_RANGE_SLOTS", "256")    # a long stream by this measure: 256-slot ranges, most of them pulled from the counter
    elif mode == "recompact_three_launches":
        monkeypatch.setenv("MIP_TUNE_TRI_BLOCK_MAX", "0")
        monkeypatch.setenv("MIP_TUNE_TRI_RECOMPACT_LAUNCHES", "3")  # round 4's count / scan / scatter instead of the one-launch re-compaction
    elif mode in ("ranges_or_sorted_waves", "sorted_waves", "ranges_of_a_large_frame"):
        monkeypatch.setenv("MIP_TUNE_TRI_BLOCK_MAX", "0")        # the large-frame path: prepare + scatter kernels, one grid, the decomposition chosen on the device ...
        if mode == "sorted_waves":
            monkeypatch.setenv("MIP_TUNE_TRI_CHOICE", "waves")   # ... forced to the wave-per-command grid
        elif mode == "ranges_of_a_large_frame":
            monkeypatch.setenv("MIP_TUNE_TRI_CHOICE", "block")   # ... forced to the range kernel's
            monkeypatch.setenv("MIP_TUNE_TRI_RANGE_SLOTS", "512")
    else:
        monkeypatch.setenv("MIP_TUNE_TRI_CHUNKS_FROM", "4294967295")  # the round-4 kernels
    if mode in ("wave", "wave_only", "tickets", "tickets_x4"):
        monkeypatch.setenv("MIP_TUNE_TRI_BLOCK_MAX", "0")   # the large-frame path: both grids, one chosen on the device ...
        monkeypatch.setenv("MIP_TUNE_TRI_PARTS_MAX", "0")
        if mode == "wave":
            monkeypatch.setenv("MIP_TUNE_TRI_CHOICE", "waves")  # ... forced to the wave-per-command grid
        elif mode == "wave_only":
            monkeypatch.setenv("MIP_TUNE_TRI_NO_CHOICE", "1")   # the second grid is not launched at all
        else:
            monkeypatch.setenv("MIP_TUNE_TRI_CHOICE", "block")  # ... to the ticket-pulling workgroup grid
            if mode == "tickets_x4":
                monkeypatch.setenv("MIP_TUNE_TRI_BATCH_FROM", "100")  # four consecutive commands per ticket (default: from 65 536 commands)
    elif mode == "parts":  # 16 work items per command (small frames), forced onto this larger frame
        monkeypatch.setenv("MIP_TUNE_TRI_PARTS_MAX", "100000000")
    else:
        monkeypatch.setenv("MIP_TUNE_TRI_BLOCK_MAX", "100000000")
        monkeypatch.setenv("MIP_TUNE_TRI_BLOCK_THREADS", mode[5:])
