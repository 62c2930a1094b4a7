"""A test-only allocator seam: what the library computes must not depend on what its buffers held.

The C ABI allocates no device memory: every scratch byte is a workspace of the caller's, many outputs
double as accumulators, and nothing says what those bytes hold on entry.  The Python wrappers take every
workspace and output from torch.empty, which under pytest hands back either fresh zeroed pages or the
block the previous identical call released — a correct answer for the same shape.  dirty() replaces the
name `torch` inside the wrapper modules with a forwarding proxy whose empty / empty_like / empty_strided,
for a DEVICE tensor, return

  a contiguous view at bytes [256, 256 + nbytes) of one uint8 allocation of nbytes + 512 bytes, the
  allocation's base asserted 256-byte aligned (the library rejects workspaces that are not), the whole
  block filled as `fill` says, the device synchronised before the view is returned (the fill is then
  ordered before every stream a call forks later).

Everything else passes through untouched: zeros, host and pinned allocations, every other attribute.
The proxy keeps every block it issued; check_guards() asserts that the 256 bytes on both sides of every
block still hold their fill — the overrun check of test_gpu_loss_workspace.Guarded, for every buffer of
every call, outputs included.

Fills
  'zero'   0x00: the clean baseline, through the same proxy, so that a clean and a dirty run differ in
           the fill only;
  'ones'   0xFF: NaN as fp32 and fp64, -1 as int32, all-ones counters and keys;
  'a5'     0xA5: a huge counter, a denormal-sized float (the fill of test_gpu_loss_workspace.py);
  stale(image)   the k-th allocation starts as the bytes of the k-th block of a recorded earlier run,
           repeated cyclically to length (and cycling over the blocks when the recorded run made fewer):
           an arena reused across calls of other shapes.  The recorder is the same proxy with
           fill='zero': image() copies its blocks after the run.

The seam covers cmhse_amd.ops, layers, evaluation, model, decoder, loss and parallel_eval: every site of
theirs that creates uninitialised device memory resolves `torch` through the module's global name
(tests/test_dirty_alloc_cpu.py walks their syntax trees and fails on a site that does not).  Not covered
by design: cmhse_amd.collate's device staging block (not in the list: the one copy that follows
overwrites all of it; pass modules=MODULES + ('cmhse_amd.collate',) to include it), tensors a TEST
allocates itself, and torch's own allocations behind autograd (zeros_like / clone of gradients), which
are initialised by definition.  `host=True` makes the proxy treat CPU tensors the same way — for the
CPU tests of this helper only."""
import importlib

import torch as _torch

GUARD = 256
MODULES = ('cmhse_amd.ops', 'cmhse_amd.layers', 'cmhse_amd.evaluation', 'cmhse_amd.model',
           'cmhse_amd.decoder', 'cmhse_amd.loss', 'cmhse_amd.parallel_eval')
BYTE = {'zero': 0x00, 'ones': 0xFF, 'a5': 0xA5}


class stale(object):
  """The fill that replays a recorded run: `image` is DirtyTorch.image()'s list of uint8 CPU tensors."""

  def __init__(self, image):
    self.blocks = [b for b in image if b.numel() > 0]
    assert self.blocks, 'the recorded run allocated nothing'

  def bytes_for(self, k, n):
    src = self.blocks[k % len(self.blocks)]
    return src.repeat(-(-n // src.numel()))[:n]


def _numel(shape):
  n = 1
  for s in shape:
    n *= int(s)
  return n


class DirtyTorch(object):
  """Stands in for the module `torch` inside the wrapper modules (see the module docstring)."""

  def __init__(self, fill, host=False):
    assert isinstance(fill, stale) or fill in BYTE, fill
    self._fill = fill
    self._host = host
    self.blocks = []           # (whole uint8 block, nbytes, the fill of the whole block or None = a byte)

  def __getattr__(self, name):
    return getattr(_torch, name)

  # ---- the three creators of uninitialised memory ---------------------------------------------------
  def _handles(self, device, pin_memory):
    if pin_memory:
      return False
    dev = _torch.device(device) if device is not None else _torch.empty(0).device
    return dev.type != 'cpu' or self._host

  def _issue(self, shape, dtype, device):
    dtype = _torch.get_default_dtype() if dtype is None else dtype
    shape = tuple(int(s) for s in shape)
    assert all(s >= 0 for s in shape), shape
    nbytes = _numel(shape) * _torch.empty(0, dtype=dtype).element_size()
    total = nbytes + 2 * GUARD
    k = len(self.blocks)
    want = self._fill.bytes_for(k, total) if isinstance(self._fill, stale) else None
    if device.type == 'cpu':      # (host=True: the host allocator aligns to 64 bytes; cut an aligned block out)
      raw = _torch.empty(total + 256, dtype=_torch.uint8)
      shift = -raw.data_ptr() % 256
      block = raw[shift:shift + total]
    else:
      block = _torch.empty(total, dtype=_torch.uint8, device=device)
    if want is None:
      block.fill_(BYTE[self._fill])
    else:
      block.copy_(want)
    assert block.data_ptr() % 256 == 0, 'the allocator returned a block that is not 256-byte aligned'
    if block.is_cuda:
      _torch.cuda.synchronize(block.device)
    self.blocks.append((block, nbytes, want))
    return block[GUARD:GUARD + nbytes].view(dtype).view(shape)

  def empty(self, *size, **kw):
    if len(size) == 1 and isinstance(size[0], (tuple, list, _torch.Size)):
      size = tuple(size[0])
    device, pin = kw.get('device'), kw.get('pin_memory', False)
    plain = set(kw) <= {'dtype', 'device', 'pin_memory', 'requires_grad'} and not kw.get('requires_grad', False)
    if not plain or not self._handles(device, pin):
      return _torch.empty(*size, **kw)
    return self._issue(size, kw.get('dtype'), _torch.device(device) if device is not None else _torch.device('cpu'))

  def empty_like(self, t, **kw):
    device = kw.get('device', t.device)
    plain = set(kw) <= {'dtype', 'device'}
    if not plain or not self._handles(device, False):
      return _torch.empty_like(t, **kw)
    return self._issue(t.shape, kw.get('dtype', t.dtype), _torch.device(device))

  def empty_strided(self, size, stride, **kw):
    device, pin = kw.get('device'), kw.get('pin_memory', False)
    plain = set(kw) <= {'dtype', 'device', 'pin_memory'}
    if not plain or not self._handles(device, pin):
      return _torch.empty_strided(size, stride, **kw)
    # (a contiguous view, as the seam promises: the wrappers only ever pass contiguous strides)
    want = _torch.empty(tuple(size), device='meta').stride()
    assert tuple(stride) == tuple(want) or _numel(size) == 0, 'empty_strided: contiguous strides only'
    return self._issue(size, kw.get('dtype'), _torch.device(device) if device is not None else _torch.device('cpu'))

  # ---- what a test asks afterwards -------------------------------------------------------------------
  def check_guards(self, where):
    """Every block's 256 bytes in front and behind still hold their fill."""
    if any(b.is_cuda for b, _, _ in self.blocks):
      _torch.cuda.synchronize()
    for k, (block, nbytes, want) in enumerate(self.blocks):
      front, back = block[:GUARD], block[GUARD + nbytes:]
      if want is None:
        byte = BYTE[self._fill]
        ok_front, ok_back = bool((front == byte).all()), bool((back == byte).all())
      else:
        w = want.to(block.device)
        ok_front = _torch.equal(front, w[:GUARD])
        ok_back = _torch.equal(back, w[GUARD + nbytes:])
      assert ok_front, '%s: allocation %d (%d bytes): something wrote in front of it' % (where, k, nbytes)
      assert ok_back, '%s: allocation %d (%d bytes): something wrote past its end' % (where, k, nbytes)

  def image(self):
    """The bytes every block holds now (between its guards), as uint8 CPU tensors: stale()'s input."""
    if any(b.is_cuda for b, _, _ in self.blocks):
      _torch.cuda.synchronize()
    return [block[GUARD:GUARD + nbytes].cpu().clone() for block, nbytes, _ in self.blocks]

  def release(self):
    self.blocks = []


def dirty(monkeypatch, fill, modules=MODULES, host=False):
  """Install a DirtyTorch as the name `torch` of `modules` (undone by monkeypatch) and return it."""
  proxy = DirtyTorch(fill, host=host)
  for name in modules:
    mod = importlib.import_module(name)
    assert getattr(mod, 'torch', None) is not None, '%s has no module-level name `torch`' % name
    monkeypatch.setattr(mod, 'torch', proxy)
  return proxy

