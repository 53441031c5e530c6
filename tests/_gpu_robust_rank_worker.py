"""Worker for the 2-rank robust sweep in tests/test_gpu_robust.py: both ranks drive the test box's one GPU, the collectives ride
the host relay (RCCL refuses duplicate devices).  Each rank reduces its own disturbance planes; the all-reduces and the worst-d
exchange are the multi-GPU path."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)


def main():
    rank, world, port, out_path, spec = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3], sys.argv[4], json.loads(sys.argv[5])
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=port, RANK=str(rank), WORLD_SIZE=str(world))
    import safebo_amd
    from safebo_amd import distributed
    from test_gpu_robust import make_model

    dist = distributed.init_from_env()
    eng = safebo_amd.SweepEngine(0)
    if spec.get("tie"):                                # a tests/tie_cases.py mirror model (mirrored in the sharded axis), exact kernel
        import tie_cases
        ds, lo, hi = tie_cases.mirror_model(q=spec["q"]), np.array(spec["lo"]), np.array(spec["hi"])
        eng.set_option("bilinear", 0)
        eng.set_option("tensor_cheb", 0)
    else:
        ds, lo, hi = make_model(spec["d"], spec["q"], spec["n"], spec["seed"])
    distributed.join(eng, dist, relay=True)
    eng.set_model(ds, mean_prior=np.zeros(spec["q"]))
    eng.set_grid_sharded(lo, hi, spec["count"])
    res = eng.sweep_robust(spec["b"], spec["nca"], spec["kind"])
    f, g = eng.robust_arrays()
    if rank == 0:
        np.savez(out_path, f=f, g=g, **{k: np.asarray(v) for k, v in res.items()})
    dist.barrier()
    eng.close()
    dist.destroy()


if __name__ == "__main__":
    main()
