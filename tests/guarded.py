"""An output buffer for the kernel tests: prefilled with a NaN / sentinel pattern and framed by guard elements of the same pattern, so that
an element the kernel left out and a write outside the result both show."""
import torch

GUARD = 64
_PATTERN = {torch.bfloat16: (torch.int16, 0x7FA5), torch.uint8: (torch.uint8, 0xA5), torch.float32: (torch.int32, 0x7FC00A5A)}


class Guarded:
    """an output buffer of n elements prefilled with a NaN / sentinel pattern, with GUARD elements of the same pattern on either side"""

    def __init__(self, n, dtype):
        self.itype, self.pat = _PATTERN[dtype]
        self.n, self.dtype = n, dtype
        self.raw = torch.full((n + 2 * GUARD,), self.pat, dtype=self.itype, device="cuda")

    def ptr(self):
        return self.raw[GUARD:].data_ptr()

    def fetch(self):
        """(typed result, its raw patterns) on the host, after checking both guards"""
        torch.cuda.synchronize()
        h = self.raw.cpu()
        assert bool((h[:GUARD] == self.pat).all()) and bool((h[GUARD + self.n:] == self.pat).all()), "wrote outside the output"
        body = h[GUARD:GUARD + self.n].clone()
        return (body if self.dtype == torch.uint8 else body.view(self.dtype)), body

    def untouched(self):
        return bool((self.fetch()[1] == self.pat).all())
