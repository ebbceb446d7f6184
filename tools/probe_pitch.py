"""Time hbk_pitch_shift on a batch of clips (HIP events on the current stream).
usage: python tools/probe_pitch.py [n_clips] [iters] [--placed] [--full-length]
       python tools/probe_pitch.py [n_clips] [iters] --alternate ROUNDS [--parent-lib PATH]

Default: full-length synthetic_clips (no silence). --placed: the bench's
clips, speech_clips (half positives, half adversarials) placed at
target_length_offsets into 23,040 samples, a quarter of them through
seven_band_eq first (its ringing extends the trailing support). Every timed
call starts from the same input (the shift runs on a fresh copy).

--alternate runs both cases in fresh child processes, ROUNDS times in turn:
[the library --parent-lib names,] the default library, and the default library
with HBK_PS_SPAN=0 (the switch is read on every call; a fresh process per
case keeps the timings independent of one another)."""
import os
import subprocess
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
flags = sys.argv[1:]


def _opt(name):
    return flags[flags.index(name) + 1] if name in flags else None


_values = {flags.index(o) + 1 for o in ("--alternate", "--parent-lib") if o in flags}
args = [a for i, a in enumerate(flags) if not a.startswith("--") and i not in _values]

if "--alternate" in flags:
    rounds = int(_opt("--alternate"))
    parent = _opt("--parent-lib")
    pos = args
    env = {k: v for k, v in os.environ.items() if k not in ("HBK_PS_SPAN", "HBK_LIB")}
    runs = ([("parent", dict(env, HBK_LIB=os.path.abspath(parent)))] if parent else []) + \
        [("span", env), ("span=0", dict(env, HBK_PS_SPAN="0"))]
    for r in range(rounds):
        for tag, e in runs:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), *pos[:2], "--placed", "--full-length"],
                               env=e, capture_output=True, text=True, timeout=600)
            if p.returncode != 0:
                sys.exit(f"{tag}: exit {p.returncode}\n{p.stdout[-2000:]}\n{p.stderr[-2000:]}")
            for line in p.stdout.splitlines():
                print(f"round {r} {tag:7s} {line}", flush=True)
    sys.exit(0)

sys.path[:0] = [ROOT, os.path.join(ROOT, "hey-buddy_amd")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

from heybuddy.kernels import pitch_shift  # noqa: E402

n = int(args[0]) if len(args) > 0 else 128
iters = int(args[1]) if len(args) > 1 else 10
T = 23040


def placed_clips():
    from heybuddy.dataset.augmented import eq_coefficients, eq_parameters, target_length_offsets
    from heybuddy.kernels import place_clips, seven_band_eq
    from heybuddy.synthetic import speech_clips
    dev = torch.device("cuda", 0)
    np.random.seed(2024)
    pos, pos_len = speech_clips("hello world", n // 2, seed=11, device=dev)
    adv, adv_len = speech_clips("hello world", n - n // 2, seed=12, device=dev, adversarial=True)
    lens = np.concatenate([pos_len, adv_len]).astype(np.int32)
    order = np.random.permutation(n)  # positives and adversarials mixed, as a shuffled batch is
    pre = target_length_offsets(lens, T)
    x0 = place_clips(torch.cat([pos, adv]), torch.from_numpy(lens), torch.from_numpy(pre.astype(np.int32)), T)
    x0 = x0[torch.from_numpy(order).to(dev)].contiguous()
    eq = np.arange(0, n, 4, dtype=np.int32)
    seven_band_eq(x0, torch.from_numpy(eq_coefficients(eq_parameters(len(eq), 6.0))), idx=torch.from_numpy(eq))
    return x0, f"placed speech_clips ({float((x0 != 0).float().mean()):.2f} non-zero)"


def full_clips():
    from heybuddy.synthetic import synthetic_clips
    return synthetic_clips(n, length=T, seed=3).cuda(), "full-length synthetic_clips"


def probe(x0, case):
    idx = torch.arange(n, dtype=torch.int32, device="cuda")
    x = torch.empty_like(x0)
    for num, den in ((128, 125), (125, 128)):
        x.copy_(x0)
        pitch_shift(x, idx, num, den, out=x)
        torch.cuda.synchronize()
        ms = 0.0
        for _ in range(iters):
            x.copy_(x0)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            pitch_shift(x, idx, num, den, out=x)
            e1.record()
            torch.cuda.synchronize()
            ms += e0.elapsed_time(e1) / iters
        print(f"pitch {num}/{den}: {case}: {n} clips {ms:.3f} ms -> {ms * 1e3 / n:.2f} us/clip", flush=True)
        if os.environ.get("HBK_LIB", "").endswith("libhbk_phase.so"):  # vocoder phase cycles (wave 0 per block)
            import ctypes
            from heybuddy._native import lib
            buf = (ctypes.c_ulonglong * 32)()
            fn = lib().hbk_debug_aug_phase
            fn.argtypes = [ctypes.c_void_p]
            fn(buf)
            x.copy_(x0)
            pitch_shift(x, idx, num, den, out=x)
            torch.cuda.synchronize()
            fn(buf)
            names = ["init", "refill", "frames", "G->LDS+barrier", "istft"]
            tot = sum(buf[16 + i] for i in range(5))
            blocks = (n + 1) // 2  # HBK_PV_CLIPS (2)
            print("  vocoder phases: " + " ".join(f"{names[i]}={buf[16 + i] / tot * 100:.1f}%" for i in range(5))
                  + f"  {tot / blocks:.0f} cyc/block (wave 0)", flush=True)


if "--full-length" in flags or "--placed" not in flags:
    probe(*full_clips())
if "--placed" in flags:
    probe(*placed_clips())
