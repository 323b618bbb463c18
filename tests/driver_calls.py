"""What tests/test_host_driver_calls.py and tests/golden/make_driver_calls.py share: the build of host/fs3d_run.cpp against the
recording stand-in tests/fs3d_stub.cpp, the matrix of command lines, and the record one run leaves (return code, stderr, masked
stdout, the per-context call logs, the sha256 of the files written).  No GPU, no libfs3d_hip.so of the package."""
import hashlib
import os
import re
import shutil
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HOST = os.path.join(ROOT, "cmc_fluid_solver_amd", "host")
DRIVER_SRC = os.path.join(HOST, "fs3d_run.cpp")
INPUTS = os.path.join(HERE, "golden", "inputs")
GOLDEN = os.path.join(HERE, "golden", "driver_calls")
TIMEOUT = 120                                     # per run, seconds: a hang is a failure

# every line of the driver that prints a host-clock number, and nothing else
MASKS = [
    (r"\(\d+ h \d+ m \d+ s left\)", "(# h # m # s left)"),
    (r"steps in (?:[0-9.]+|inf) s: (?:[0-9.]+|inf|-?nan) Mcells/s", "steps in # s: # Mcells/s"),
    (r"(Moving geometry per step \(host clock, ms\)): Prepare [0-9.]+, extrusion on the host [0-9.]+, update call [0-9.]+; step [0-9.]+",
     r"\1: Prepare #, extrusion on the host #, update call #; step #"),
    (r"(Moving mesh per step \(host clock, ms\)): SubFrame [0-9.]+, voxels on the host [0-9.]+, update call [0-9.]+; step [0-9.]+",
     r"\1: SubFrame #, voxels on the host #, update call #; step #"),
    # Moving mesh, both paths: the three host clocks; `its device time` is the stand-in's constant and stays
    (r"(host voxels \+ fs3d_update_nodes|fs3d_update_nodes_shape3d|time step) median [0-9.]+ min [0-9.]+ max [0-9.]+", r"\1 median # min # max #"),
    (r"(Result output per record \(host clock, ms\)): GetLayer [0-9.]+, AppendLayer [0-9.]+;", r"\1: GetLayer #, AppendLayer #;"),
]


def mask(text):
    for pat, rep in MASKS:
        text = re.sub(pat, rep, text)
    return text


def build(outdir, sanitize=False):
    """libfs3d_hip.so (the stand-in) and fs3d_run in `outdir`, the driver with the flags of build.build_driver; rpath $ORIGIN."""
    os.makedirs(outdir, exist_ok=True)
    cxx = os.environ.get("CXX", "g++")
    san = ["-fsanitize=thread", "-O1", "-g"] if sanitize else []
    subprocess.check_call([cxx, "-std=c++17", "-O2", "-Wall", "-shared", "-fPIC"] + san +
                          [os.path.join(HERE, "fs3d_stub.cpp"), "-o", os.path.join(outdir, "libfs3d_hip.so")])
    exe = os.path.join(outdir, "fs3d_run")
    subprocess.check_call([cxx, "-std=c++17", "-O2", "-Wall", "-ffp-contract=off"] + san + ["-I" + os.path.join(ROOT, "include"), DRIVER_SRC, "-o", exe,
                           "-L" + outdir, "-lfs3d_hip", "-lz", "-Wl,-rpath,$ORIGIN", "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def _case(inp, words, fail=None, config=None):
    return {"input": inp, "words": words.split(), "fail": fail, "config": config}


B, H, S, W = "box_pipe_2D", "heart_us_2D", "sphere_3D", "white_sea"
RUNS = {
    "box": _case(B, "GPU --steps 11"),
    "box_csv": _case(B, "GPU CSV --steps 11"),
    "box_double": _case(B, "GPU double --steps 11"),
    "box_2slabs": _case(B, "GPU 2 --same-device --steps 11"),
    "box_3devices": _case(B, "GPU 3 --steps 11"),
    "box_steps0": _case(B, "GPU --steps 0"),
    "box_time_output": _case(B, "GPU --time-output --steps 11"),
    "box_filter_box": _case(B, "GPU --output-filter box --steps 11"),
    "box_device1": _case(B, "GPU --device 1 --steps 11"),
    # 10 frames of 3 steps: 5 steps cross a frame boundary (the substep counter restarts)
    "heart": _case(H, "GPU --steps 5"),
    "heart_moving": _case(H, "GPU moving --steps 5"),
    "heart_moving_host_timed": _case(H, "GPU moving --host-extrusion --time-geometry --steps 5"),
    "heart_moving_fresh": _case(H, "GPU moving --fresh-cells --steps 5"),
    "heart_moving_2slabs": _case(H, "GPU 2 --same-device moving --steps 5"),
    "heart_moving_host_3slabs": _case(H, "GPU 3 --same-device moving --host-extrusion --steps 5"),
    "heart_moving_fresh_2slabs": _case(H, "GPU 2 --same-device moving --slab-fresh-cells --steps 5"),
    "sphere_mesh": _case(S, "GPU moving-mesh --steps 6"),
    "sphere_mesh_host": _case(S, "GPU moving-mesh --host-voxels --steps 6"),
    "sphere_mesh_both": _case(S, "GPU moving-mesh --time-both --steps 6"),
    "sphere_mesh_host_both": _case(S, "GPU moving-mesh --host-voxels --time-both --steps 6"),
    "sphere_mesh_walls_fresh": _case(S, "GPU moving-mesh --watertight --thin-shell --wall-velocity motion --wall-temperature 1.5 --fresh-cells --steps 6"),
    "sphere_mesh_wall_file": _case(S, "GPU moving-mesh --watertight --wall-velocity file --steps 6"),
    "sphere_mesh_host_2slabs": _case(S, "GPU 2 --same-device moving-mesh --host-voxels --steps 6"),
    "sphere_mesh_slab_voxels": _case(S, "GPU 2 moving-mesh --slab-voxels --steps 6"),
    "sphere_mesh_slab_voxels_wallT": _case(S, "GPU 2 moving-mesh --slab-voxels --watertight --wall-temperature 2 --steps 6"),
    "sphere_mesh_slab_voxels_3slabs_fresh": _case(S, "GPU 3 moving-mesh --slab-voxels --watertight --wall-velocity motion --slab-fresh-cells --steps 6"),
    "white_sea": _case(W, "GPU --steps 2"),                       # the depth variable of the result header
    # the failure hook: the failing rank's own message, not `another slab thread failed`
    "fail_step3": _case(B, "GPU --steps 11", fail="fs3d_time_step:0:3"),
    "fail_step3_rank1_of_3": _case(B, "GPU 3 --steps 11", fail="fs3d_time_step:22:3"),        # 64 planes in 3 slabs: rank 1 starts at plane 22
    "fail_slab_voxels_rank0_call2": _case(S, "GPU 2 moving-mesh --slab-voxels --steps 6", fail="fs3d_update_nodes_shape3d_slab:0:2"),
    # no context: one GPU leaves no result file, GPU n has created it before its threads start
    "fail_create": _case(B, "GPU --steps 11", fail="fs3d_create:0:1"),
    "fail_create_rank1_of_2": _case(B, "GPU 2 --same-device --steps 11", fail="fs3d_create:32:1"),
}
for _tag, _gpu in (("", "GPU"), ("_2slabs", "GPU 2 --same-device")):
    RUNS["stats_mean" + _tag] = _case(B, _gpu + " --time-stats mean --steps 7")
    RUNS["stats_variance" + _tag] = _case(B, _gpu + " --time-stats variance --steps 7")
    RUNS["stats_cov_every2" + _tag] = _case(B, _gpu + " --time-stats variance --time-covariances --time-stats-every 2 --steps 7")
    RUNS["stats_mean_steps0" + _tag] = _case(B, _gpu + " --time-stats mean --steps 0")

# the multi-slab moving and statistics runs that are repeated under ThreadSanitizer
TSAN_RUNS = ["heart_moving_host_3slabs", "heart_moving_fresh_2slabs", "sphere_mesh_host_2slabs", "sphere_mesh_slab_voxels_3slabs_fresh",
             "stats_cov_every2_2slabs"]

# one case per refusal of run() and main(): name -> (case, the text of the std::runtime_error site it reaches)
_BOX_CFG = "box_pipe_2D_config.txt"
REFUSALS = {
    "refuse_moving_not_shape2d": (_case(S, "GPU moving"), "moving: only in_fmt Shape2D inputs move"),
    "refuse_moving_devices": (_case(H, "GPU 2 moving"), "moving: single GPU only, or GPU n with --same-device"),
    "refuse_host_extrusion_alone": (_case(B, "GPU --host-extrusion"), "--host-extrusion: only with moving"),
    "refuse_mesh_not_shape3d": (_case(B, "GPU moving-mesh"), "moving-mesh: only in_fmt Shape3D inputs are meshes"),
    "refuse_slab_voxels_alone": (_case(B, "GPU 2 --slab-voxels"), "--slab-voxels: only with moving-mesh"),
    "refuse_slab_voxels_one_gpu": (_case(S, "GPU moving-mesh --slab-voxels"), "--slab-voxels: only with GPU n for n > 1"),
    "refuse_slab_and_host_voxels": (_case(S, "GPU 2 moving-mesh --slab-voxels --host-voxels"), "--slab-voxels: not together with --host-voxels"),
    "refuse_mesh_slabs_on_device": (_case(S, "GPU 2 moving-mesh"), "moving-mesh: the device voxelisation runs on a single GPU only"),
    "refuse_timing_words_on_slabs": (_case(S, "GPU 2 moving-mesh --host-voxels --time-both"), "--time-both, --time-geometry: single GPU only"),
    "refuse_host_voxels_alone": (_case(B, "GPU --host-voxels"), "--host-voxels: only with moving-mesh"),
    "refuse_time_both_alone": (_case(B, "GPU --time-both"), "--time-both: only with moving-mesh"),
    "refuse_time_geometry_alone": (_case(B, "GPU --time-geometry"), "--time-geometry: only with moving or moving-mesh"),
    "refuse_watertight_not_mesh": (_case(B, "GPU --watertight"), "--watertight: only in_fmt Shape3D inputs are meshes"),
    "refuse_wall_velocity_not_mesh": (_case(B, "GPU --wall-velocity motion"), "--wall-velocity: only in_fmt Shape3D inputs are meshes"),
    "refuse_thin_shell_alone": (_case(S, "GPU --thin-shell"), "--thin-shell: needs --watertight"),
    "refuse_wall_velocity_not_watertight": (_case(S, "GPU --wall-velocity motion"), "--wall-velocity: needs --watertight"),
    "refuse_wall_temperature_not_mesh": (_case(B, "GPU --wall-temperature 1"), "--wall-temperature: only in_fmt Shape3D inputs are meshes"),
    "refuse_wall_temperature_inf": (_case(S, "GPU --wall-temperature inf"), "--wall-temperature: not a finite number"),
    "refuse_wall_temperature_moving_open": (_case(S, "GPU moving-mesh --wall-temperature 1"), "--wall-temperature: a moving-mesh run needs --watertight"),
    "refuse_walls_time_both": (_case(S, "GPU moving-mesh --watertight --wall-temperature 1 --time-both"), "--time-both: not together with --wall-velocity"),
    "refuse_fresh_cells_alone": (_case(B, "GPU --fresh-cells"), "--fresh-cells: only with moving or moving-mesh"),
    "refuse_fresh_cells_slabs": (_case(H, "GPU 2 --same-device moving --fresh-cells"), "--fresh-cells: single GPU only"),
    "refuse_fresh_cells_time_both": (_case(S, "GPU moving-mesh --fresh-cells --time-both"), "--fresh-cells: not together with --time-both"),
    "refuse_grid_time_sea": (_case(W, "GPU --grid-time 0.5"), "--grid-time: only in_fmt Shape2D and Shape3D inputs move"),
    "refuse_grid_only_path": (_case(B, "GPU --grid-only no_such_directory/grid.bin"), "cannot create "),
    "refuse_dimension": (_case(B, "GPU", config=("cavity_2D_config.txt", None, None)), "only `dimension 3D` runs are supported"),
    "refuse_in_fmt": (_case(B, "GPU", config=(_BOX_CFG, r"in_fmt\s+Shape2D", "in_fmt Shape4D")), ": unknown input format"),
    "refuse_frame_time": (_case(S, "GPU", config=("sphere_3D_config.txt", r"frame_time\s+\S+", "")), "must specify frame time!"),
    "refuse_solver": (_case(B, "GPU", config=(_BOX_CFG, r"solver\s+ADI", "solver Stable")), " is not implemented (the reference implements ADI only)"),
    "refuse_wall_velocity_word": (_case(S, "GPU --wall-velocity fast"), "--wall-velocity: motion or file"),
    "refuse_wall_temperature_missing": (_case(S, "GPU --wall-temperature"), "--wall-temperature: a number follows"),
    "refuse_wall_temperature_word": (_case(S, "GPU --wall-temperature warm"), "--wall-temperature: not a number"),
    "refuse_output_filter_word": (_case(B, "GPU --output-filter gauss"), "--output-filter: point or box"),
    "refuse_time_stats_word": (_case(B, "GPU --time-stats median"), "--time-stats: mean or variance"),
    "refuse_time_stats_every": (_case(B, "GPU --time-stats mean --time-stats-every 0"), "--time-stats-every: an integer from 1 to 1048576 follows"),
    "refuse_covariances_alone": (_case(B, "GPU --time-stats mean --time-covariances"), "--time-covariances: needs --time-stats variance"),
    "refuse_filter_box_slabs": (_case(B, "GPU 2 --same-device --output-filter box"), "--output-filter box: single GPU only"),
}
# std::runtime_error sites of fs3d_run.cpp that no command line reaches, each with the reason
NOT_A_REFUSAL = {
    "moving-mesh: not together with moving": "moving needs in_fmt Shape2D and moving-mesh in_fmt Shape3D: one of those two refusals comes first",
    "another slab thread failed": "the barrier's own text for the ranks a failing rank releases; the fail_* runs check that it is NOT what the driver reports",
}
CASES = dict(RUNS, **{k: v[0] for k, v in REFUSALS.items()})


def run_case(exe, case, workdir):
    """Run one command line in an empty `workdir` (the prefix is the relative `out`, so no path of this machine is printed)."""
    if os.path.isdir(workdir):
        shutil.rmtree(workdir)
    os.makedirs(workdir)
    cfg = os.path.join(INPUTS, case["input"] + "_config.txt")
    if case["config"]:
        base, pat, rep = case["config"]
        text = open(os.path.join(INPUTS, base)).read()
        if pat:
            assert re.search(pat, text), pat
            text = re.sub(pat, rep, text)
        cfg = os.path.join(workdir, "config.txt")
        with open(cfg, "w") as f:
            f.write(text)
    data = os.path.join(INPUTS, case["input"] + ("_data.nc" if case["input"] == W else "_data.txt"))
    env = dict(os.environ, FS3D_STUB_LOG=os.path.join(workdir, "calls"))
    env.pop("FS3D_STUB_FAIL", None)
    if case["fail"]:
        env["FS3D_STUB_FAIL"] = case["fail"]
    r = subprocess.run([exe, data, "out", cfg, "align"] + case["words"], cwd=workdir, env=env, capture_output=True, text=True, timeout=TIMEOUT)
    logs = {f.split(".", 1)[1]: open(os.path.join(workdir, f)).read() for f in sorted(os.listdir(workdir)) if f.startswith("calls.")}
    files = {}
    for name in ("out_res.nc", "out_stats.nc"):
        path = os.path.join(workdir, name)
        files[name] = hashlib.sha256(open(path, "rb").read()).hexdigest() if os.path.exists(path) else None
    return {"words": ["align"] + case["words"], "fail": case["fail"], "returncode": r.returncode, "stderr": r.stderr, "stdout": mask(r.stdout),
            "logs": logs, "files": files}

