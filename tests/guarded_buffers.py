"""Device buffers between two 4 KB bands of a pattern, for the tests that check that an entry point stores nothing outside its
workspace or its outputs (tests/test_gpu_mvar_measures.py, tests/test_gpu_workspace_guards.py): single buffers, and a memory
adapter for the stage-D drivers (spectral_connectivity_amd/_stage_d.py) whose every array is such a buffer."""
import functools

BAND = 4096
FILL = 0x5A


@functools.lru_cache(maxsize=None)
def pattern():
    import torch
    return torch.arange(BAND, dtype=torch.int32, device="cuda:0").mul_(37).add_(11).to(torch.uint8)


def guarded(n):
    """uint8 [BAND + n + BAND]: n payload bytes of FILL (256-aligned) between the two bands"""
    import torch
    buf = torch.empty(n + 2 * BAND, dtype=torch.uint8, device="cuda:0")
    buf[BAND:BAND + n] = FILL
    buf[:BAND] = pattern()
    buf[BAND + n:] = pattern()
    assert (buf.data_ptr() + BAND) % 256 == 0
    return buf


def intact(buf, n):
    import torch
    return bool(torch.equal(buf[:BAND], pattern())) and bool(torch.equal(buf[BAND + n:], pattern()))


def guarded_memory():
    """engine.TorchMemory on cuda:0 whose ``empty`` arrays -- the workspace and the outputs of a stage-D driver -- are payloads of
    guarded buffers: ``sizes()`` their byte counts, ``intact()`` every band survived, ``untouched()`` every payload is still FILL."""
    import torch
    from spectral_connectivity_amd import engine

    class GuardedMemory(engine.TorchMemory):
        def __init__(self):
            super().__init__(torch.device("cuda:0"))
            self.buffers = []

        def empty(self, shape, dtype):
            like = torch.empty(shape, dtype=engine._TORCH_DTYPES[dtype], device="meta")
            n = like.numel() * like.element_size()
            self.buffers.append((guarded(n), n))
            return self.buffers[-1][0][BAND:BAND + n].view(like.dtype).view(like.shape)

        def sizes(self):
            return [n for _, n in self.buffers]

        def intact(self):
            return all(intact(buf, n) for buf, n in self.buffers)

        def untouched(self):
            return all(bool((buf[BAND:BAND + n] == FILL).all()) for buf, n in self.buffers)

    return GuardedMemory()
