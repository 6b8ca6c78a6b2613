"""GPU tests: run a piece of work in a way that fails if it synchronises with the host."""
import torch


def _sync_debug_mode_is_honoured():
    """Does this torch build raise on a synchronising call under set_sync_debug_mode("error")?"""
    x = torch.ones(1, device="cuda")
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        x.item()
    except RuntimeError:
        return True
    finally:
        torch.cuda.set_sync_debug_mode("default")
    return False


def run_without_host_sync(work):
    """What ``work()`` returns, from a call that a host synchronisation fails: under ``torch.cuda.set_sync_debug_mode("error")`` where
    this torch build honours it on ROCm (probed with an ``.item()``, which must raise); otherwise captured into a graph on a side
    stream, where a synchronisation fails the capture, and replayed once.  Which one ran is printed.  Warm the work up first
    (library, allocators); the device is synchronised before and after."""
    torch.cuda.synchronize()
    if _sync_debug_mode_is_honoured():
        print("\nmechanism: torch.cuda.set_sync_debug_mode('error')")
        torch.cuda.set_sync_debug_mode("error")
        try:
            got = work()
        finally:
            torch.cuda.set_sync_debug_mode("default")
    else:
        print("\nmechanism: stream capture (set_sync_debug_mode is not honoured by this build)")
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            got = work()
        graph.replay()
    torch.cuda.synchronize()
    return got
