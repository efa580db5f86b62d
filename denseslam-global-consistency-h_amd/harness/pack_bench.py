"""Cost of parking a local map (dslam_pack_scene, dslam_unpack_scene) on three finished S-street maps, with the two
yardsticks measured in the same run: a plain copy of the same number of bytes between device and page-locked memory, and
the path a caller had before -- the download / upload calls harness/checkpoint.py makes (table, both lists, the used slot
range of the pool, through pageable memory).

The maps are merge_bench.py's: the drive split into local maps of K keyframes, each in a scene with the default pools.
Reported per map, as wall clock per call (every call waits for the stream itself; the first repetition is not counted):
  * the packed size, n and f;
  * pack and unpack with the image in device memory, and in page-locked host memory (the unpack goes into a scene of
    n + 64 blocks, created beforehand);
  * a plain device -> page-locked copy of total_bytes and the copy back;
  * checkpoint.py's downloads and uploads and the bytes they move;
  * a compaction as ITMMainEngine::CompactLocalMap makes it: size query, pack to device memory, a new scene of n + 64
    blocks, unpack, the old scene destroyed.
Prints one JSON line; with an argument `out.json` also writes it there.

    python denseslam-global-consistency-h_amd/harness/pack_bench.py [reps] [out.json]
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(1, os.path.dirname(os.path.abspath(__file__)))
import __graft_entry__ as ge  # noqa: E402

from merge_bench import K  # noqa: E402  (the same maps)

MAPS, HEADROOM = 3, 64


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 10
    out_path = sys.argv[2] if len(sys.argv) > 2 else None
    pkg = ge.load_package()
    from dslam_amd.harness import synth
    eng = pkg.open_engine(0)
    import torch
    wl = synth.s_street(640, 480)
    W, H, intr = wl.W, wl.H, wl.intr
    p = pkg.SceneParams(**wl.scene_kwargs)
    view = eng.create_view(W, H)

    def fuse(j):
        scene = eng.create_scene(p)
        rs = eng.create_render_state(scene, W, H)
        Tinv = np.linalg.inv(np.asarray(wl.frame(j * K)[2], np.float64))
        for i in range(j * K, j * K + K):
            rgba, mm, M = wl.frame(i)
            eng.view_update(view, rgba, mm, timestamp=float(i))
            eng.process_frame(scene, view, rs, (np.asarray(M, np.float64) @ Tinv).astype(np.float32), intr)
        rs.close()
        return scene

    def timed(call, n=reps):
        times = []
        for rep in range(n + 1):
            t0 = time.perf_counter()
            call()
            if rep:
                times.append((time.perf_counter() - t0) * 1e3)
        return {"mean": float(np.mean(times)), "min": float(np.min(times)), "max": float(np.max(times))}

    rows = []
    for j in range(MAPS):
        scene = fuse(j)
        eng.synchronize()
        info = eng.pack_scene(scene)
        total, n = info.total_bytes, info.blocks
        dev = torch.empty(total, dtype=torch.uint8, device="cuda:0")
        pinned = eng.host_alloc((total,), np.uint8)
        pinned_t = torch.empty(total, dtype=torch.uint8, pin_memory=True)
        q = pkg.SceneParams(**dict(wl.scene_kwargs, num_local_blocks=n + HEADROOM))
        small = eng.create_scene(q)
        row = {"map": j, "blocks": n, "free_excess": info.free_excess, "total_bytes": total,
               "pool_bytes_before": scene.params.num_local_blocks * 4096, "pool_bytes_after": (n + HEADROOM) * 4096}
        row["pack_device_ms"] = timed(lambda: eng.pack_scene(scene, dev.data_ptr(), total))
        row["unpack_device_ms"] = timed(lambda: eng.unpack_scene(small, dev.data_ptr(), total))
        row["pack_pinned_ms"] = timed(lambda: eng.pack_scene(scene, pinned.ctypes.data, total))
        row["unpack_pinned_ms"] = timed(lambda: eng.unpack_scene(small, pinned.ctypes.data, total))
        assert bytes(pinned[:64]) == bytes(info) and np.array_equal(dev.cpu().numpy(), pinned)

        def copy_out():
            pinned_t.copy_(dev, non_blocking=True)
            torch.cuda.synchronize()

        def copy_back():
            dev.copy_(pinned_t, non_blocking=True)
            torch.cuda.synchronize()

        row["memcpy_device_to_pinned_ms"] = timed(copy_out)
        row["memcpy_pinned_to_device_ms"] = timed(copy_back)

        # the calls of checkpoint.save_map / load_map, without the file
        state = {}

        def download():
            st = eng.stats(scene)
            table = eng.download_hash_table(scene)
            used = table["ptr"][table["ptr"] >= 0]
            first = int(used.min()) if used.size else scene.params.num_local_blocks
            state.update(table=table, first=first, tops=(st["last_free_block_id"], st["last_free_excess_id"]),
                         blocks=eng.download_voxel_blocks(scene, first, scene.params.num_local_blocks - first),
                         alloc=eng.download_allocation_list(scene), excess=eng.download_excess_list(scene))

        row["checkpoint_download_ms"] = timed(download, max(2, reps // 3))
        twin = eng.create_scene(p)

        def upload():
            eng.upload_scene_state(twin, hash_table=state["table"], allocation_list=state["alloc"], last_free_block_id=state["tops"][0],
                                   excess_list=state["excess"], last_free_excess_id=state["tops"][1])
            eng.upload_voxel_blocks(twin, state["first"], state["blocks"])

        row["checkpoint_upload_ms"] = timed(upload, max(2, reps // 3))
        row["checkpoint_bytes"] = int(state["table"].nbytes + state["blocks"].nbytes + state["alloc"].nbytes + state["excess"].nbytes)
        twin.close()
        small.close()

        # one compaction, end to end (the scene is replaced: once)
        t0 = time.perf_counter()
        info2 = eng.pack_scene(scene)
        buf = torch.empty(info2.total_bytes, dtype=torch.uint8, device="cuda:0")
        eng.pack_scene(scene, buf.data_ptr(), info2.total_bytes)
        compact = eng.create_scene(q)
        eng.unpack_scene(compact, buf.data_ptr(), info2.total_bytes)
        scene.close()
        row["compact_ms"] = (time.perf_counter() - t0) * 1e3
        compact.close()
        for key in ("pack_device", "unpack_device", "pack_pinned", "unpack_pinned", "memcpy_device_to_pinned", "memcpy_pinned_to_device"):
            row[key + "_GBps"] = total / (row[key + "_ms"]["mean"] * 1e-3) / 1e9
        eng.host_free(pinned)
        del dev, pinned_t, buf
        rows.append(row)

    out = {"workload": "S-street", "image": f"{W}x{H}", "keyframes_per_map": K, "reps": reps,
           "unit": "ms per call, wall clock; measured on the part", "maps": rows}
    line = json.dumps(out)
    print(line)
    if out_path:
        with open(out_path, "w") as f:
            f.write(json.dumps(json.loads(line), indent=1) + "\n")
    view.close()
    eng.close()


if __name__ == "__main__":
    main()
