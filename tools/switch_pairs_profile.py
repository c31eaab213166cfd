"""Writes the measured distances of the switch sweep (tests/switch_pairs.py): one line per row with its levels, the token counts N of its passes,
loss and logit error, the worst gradient relative error and the lowest cosine with their tensors, the plain twin's same four figures, and the
seconds each took (model construction, passes, eval forward; the oracle apart).  Needs an MI355X.

    python tools/switch_pairs_profile.py [OUT] [SWEEP_S SUITE_WITH_S SUITE_WITHOUT_S]        (default OUT: profiles/switch_pairs.txt)

The three optional numbers are wall times in seconds that the caller measured with `time` around pytest on the same machine: of
tests/test_switch_pairs_gpu.py alone, of the whole GPU suite (-m gpu) with that file, and of the same suite with --ignore of that file (what the
suite took before the sweep existed).  Given, they become the file's last line, with what they leave of the suite driver's 900 s limit."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import torch  # noqa: E402

import switch_pairs as sp  # noqa: E402


SUITE_LIMIT_S = 900


def main(out_path, walls=None):
    from diverse_channel_vit_amd import hip
    dev = torch.device("cuda:0")
    hip.set_deterministic(True)  # as the suite's conftest does; each row sets its own level and puts this back
    t0 = time.perf_counter()
    sp.run_model(sp.rows()[0], dev)  # load the library and warm the allocator outside the timed rows
    lines, bad, t_oracle = [], 0, 0.0
    for row in sp.rows():
        t = time.perf_counter()
        ref = sp.run_oracle(row)
        t_oracle += time.perf_counter() - t
        got = sp.run_model(row, dev)
        fig, fail = sp.compare(row, ref, got)
        twin = row.plain_twin()
        tgot = sp.run_model(twin, dev)
        tfig, tfail = sp.compare(twin, ref, tgot)
        lines.append(sp.format_line(row, fig, got["seconds"], tfig, tgot["seconds"]) + ("" if not fail else "  ROW MISSES: " + "; ".join(fail))
                     + ("" if not tfail else "  TWIN MISSES: " + "; ".join(tfail)))
        bad += bool(fail) + bool(tfail)
        print(lines[-1], flush=True)
    total = time.perf_counter() - t0
    lines.append(f"total {total:.1f} s for {len(lines)} rows and their twins (fp64 oracle on the host: {t_oracle:.1f} s of it); {bad} runs outside a bound")
    print(lines[-1])
    if walls:
        sweep, with_, without = walls
        lines.append(f"tests/test_switch_pairs_gpu.py alone: {sweep:.0f} s wall.  Whole GPU suite (-m gpu, one GPU): {with_:.0f} s wall with this file, "
                     f"{without:.0f} s with --ignore of it (the suite before the sweep); {SUITE_LIMIT_S - with_:.0f} s of the driver's {SUITE_LIMIT_S} s limit "
                     f"are left.")
        print(lines[-1])
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) not in (1, 2, 5):
        sys.exit(__doc__)
    sys.exit(main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "switch_pairs.txt"),
                  [float(v) for v in sys.argv[2:5]] if len(sys.argv) == 5 else None))
