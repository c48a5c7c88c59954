"""Re-check the launch-configuration defaults of the convolution kernels on the bench: one bench.py run per setting of a
tunable (its PAI_TUNE_<name> default)."""
import json, os, subprocess, sys
SWEEP = [{}, {"PAI_TUNE_fwd_patch256": "0"}, {"PAI_TUNE_wgrad_target": "512"}, {"PAI_TUNE_wgrad_target": "1024"},
         {"PAI_TUNE_wgrad_target": "1536"}, {"PAI_TUNE_wgrad_patch": "0"}, {"PAI_TUNE_wgrad_minrows": "1024"},
         {"PAI_TUNE_thin_wgrad_blocks": "2048"}, {}]
for env in SWEEP:
    r = subprocess.run([sys.executable, "bench.py", "--steps", "30", "--warmup", "5", "--no-cpu-baseline", "--no-kernel-events"],
                       env=dict(os.environ, **env), capture_output=True, text=True)
    try:
        d = json.loads(r.stdout.strip().splitlines()[-1])
        print(f"{str(env):40s} {d['ms_per_step']:7.3f} ms  {d['value']:8.1f} img/s", flush=True)
    except Exception:
        print(env, "ERR", r.stderr[-300:], flush=True)
