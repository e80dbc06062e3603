"""HIP-event timing for the *_time.py scripts: warm-up calls, then one pair of events per repetition."""
import statistics

import torch


def times_ms(fn, reps, warm=3):
    """The times of `reps` calls of fn, in ms between two HIP events, after `warm` untimed calls."""
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return ts


def median_ms(fn, reps, warm=3):
    return statistics.median(times_ms(fn, reps, warm))
