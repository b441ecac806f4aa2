"""Output and input side of the hot path.  Output: decoded pixels -> the bytes the serving loop JPEG-encodes.

The reference's frame callback (release_server.py:978-991) copies the decoder's float32 pixels [1, T, 3, H, W] to a
pinned host tensor on a download stream (after waiting on the event recorded behind the decode), normalises them on
the CPU (`add_(1.0).mul_(0.5).clamp_(0.0, 1.0)`) and hands every frame to `TF.to_pil_image(...).save(JPEG)` (:972), whose
float path is `mul(255).byte()` in H x W x C order.  `FrameDownloader` is that callback with the arithmetic moved in front
of the copy (`rtv_pixels_to_rgb8`): the device-to-host transfer carries 1 byte per sample instead of 4 (14.4 MB instead of
57.5 MB per 12-frame block), the CPU does no arithmetic, and the result is bit-identical
(`oracle/vae_oracle.frames_to_rgb8`).  JPEG encoding / the WebSocket stay with the caller (control plane, out of scope) -
unless the caller opts into `JpegFrameDownloader`: the same call protocol, but the block is JPEG-encoded on the device
(`rtv_jpeg_encode`, csrc/jpeg_encode.hip: baseline 4:2:0 JFIF at the reference's quality 90, one restart interval per MCU row)
and only the files cross to the host, so the caller needs no CPU encode pool and `fetch` returns bytes ready to send.

Input: the reference's push_frame (release_server.py:470-487) turns every decoded camera image into a float16 tensor on the
CPU (`TF.to_tensor(image).to(float16).pin_memory()`), uploads 2 bytes per sample on an upload stream and maps it to [-1, 1]
there (`sub_(0.5).mul_(2.0)`); frames of another size than the session's are resized per block (v2v.py:153).  `FrameUploader`
is the mirror image of the downloader: the bytes go up as they are, 1 byte per sample, into a device ring of frame slots, and
one launch per block (`rtv_frames_from_rgb8`) decodes, resizes and lays out the block's frames for the encoder.  `push_jpeg` takes
what the reference's push_frame takes, the camera's JPEG file: the file goes up as it arrived (about a tenth of its pixels' bytes)
and is decoded on the device (`rtv_jpeg_decode`, csrc/jpeg_decode.hip) into the ring slot a raw frame would have landed in.
"""
import torch

from . import ops


class FrameDownloader:
    """Use as `GenerationSession(..., frame_callback=downloader)`.  Every call enqueues conversion + async copy into one
    of `slots` pinned buffers on the download stream and returns a ticket; `fetch(ticket)` waits for that copy only and
    returns uint8 [T, H, W, 3] (a view of the pinned buffer, valid until the slot is reused `slots` calls later)."""

    def __init__(self, device="cuda", slots=2):
        if slots < 1:
            raise ValueError("slots must be >= 1")
        self.device = torch.device(device)
        self.stream = torch.cuda.Stream(device=self.device)     # release_server.py:88-90 download_stream
        self.slots = slots
        self._host = [None] * slots
        self._dev = [None] * slots
        self._done = [None] * slots
        self._shape = [None] * slots
        self._frame_ids = [None] * slots
        self._n = 0

    def __call__(self, pixels, frame_ids=(), event=None):
        if pixels.dim() != 5 or pixels.shape[0] != 1 or pixels.shape[2] != 3:
            raise ValueError("expected decoder pixels [1, T, 3, H, W]")
        T, _, H, W = pixels.shape[1:]
        slot = self._n % self.slots
        if self._done[slot] is not None:
            self._done[slot].synchronize()                      # the slot's previous copy must have landed before reuse
        n = T * H * W * 3
        if self._host[slot] is None or self._host[slot].numel() < n:
            self._host[slot] = torch.empty(n, dtype=torch.uint8, pin_memory=True)
            self._dev[slot] = torch.empty(n, dtype=torch.uint8, device=self.device)
        if event is None:
            event = torch.cuda.Event()
            event.record(torch.cuda.current_stream(self.device))
        self.stream.wait_event(event)                           # :981 download_stream.wait_event(event)
        with torch.cuda.stream(self.stream):
            src = pixels[0].float().contiguous()
            src.record_stream(self.stream)
            rgb = ops.pixels_to_rgb8(src, out=self._dev[slot][:n].view(T, H, W, 3))
            self._host[slot][:n].copy_(rgb.view(-1), non_blocking=True)
            done = torch.cuda.Event()
            done.record(self.stream)
        self._done[slot], self._shape[slot], self._frame_ids[slot] = done, (T, H, W, 3), list(frame_ids)
        self._n += 1
        return self._n - 1

    def fetch(self, ticket):
        if not (self._n - self.slots <= ticket < self._n) or ticket < 0:
            raise KeyError(f"ticket {ticket} is no longer (or not yet) held; {self.slots} slots")
        slot = ticket % self.slots
        self._done[slot].synchronize()
        T, H, W, C = self._shape[slot]
        return self._host[slot][:T * H * W * C].view(T, H, W, C)

    def frame_ids(self, ticket):
        return self._frame_ids[ticket % self.slots]


class JpegFrameDownloader:
    """`FrameDownloader`'s call protocol with the JPEG encode in front of the copy: every call enqueues, on the download stream,
    one `rtv_jpeg_encode` of the block's float pixels, an async copy of the frame offsets and an async copy of the files into
    one of `slots` pinned buffers, and returns a ticket; `fetch(ticket)` waits for that slot only and returns a list of T
    memoryviews over the pinned buffer, each a complete JPEG file, valid until the slot is reused `slots` calls later.

    How many bytes a block's files take is known on the device only, so the payload copy is sized by a running estimate:
    H * W * T / 2 bytes at first, then 1.25 x the largest total seen.  `fetch` reads the true total from the offsets and copies
    the rest when the estimate fell short (one more copy and wait; the estimate grows).  The device buffer of a slot has
    `rtv_jpeg_out_bound` bytes, which the files cannot exceed, so nothing is ever encoded twice; it and the arena are cached per
    slot, and the header travels by value with the launch (nothing is uploaded)."""

    def __init__(self, device="cuda", slots=2, quality=90):
        if slots < 1:
            raise ValueError("slots must be >= 1")
        if not 1 <= int(quality) <= 100:
            raise ValueError("quality must be in 1..100")
        self.device = torch.device(device)
        self.stream = torch.cuda.Stream(device=self.device)     # release_server.py:88-90 download_stream
        self.slots, self.quality = slots, int(quality)
        self._key = [None] * slots                              # (T, H, W) the slot's device buffers are sized for
        self._arena = [None] * slots
        self._dev = [None] * slots                              # uint8 [rtv_jpeg_out_bound]
        self._offs = [None] * slots                             # int64 [T + 1] on the device
        self._host = [None] * slots                             # pinned uint8, grows with the estimate
        self._host_offs = [None] * slots                        # pinned int64 [T + 1]
        self._copied = [0] * slots
        self._done = [None] * slots
        self._frame_ids = [None] * slots
        self._largest = 0                                       # largest total of one block seen so far
        self.topups = 0                                         # fetches whose estimate fell short (each cost one more copy and wait)
        self._n = 0

    def _estimate(self, T, H, W):
        return (self._largest * 5 + 3) // 4 if self._largest else T * H * W // 2

    def __call__(self, pixels, frame_ids=(), event=None):
        if pixels.dim() != 5 or pixels.shape[0] != 1 or pixels.shape[2] != 3:
            raise ValueError("expected decoder pixels [1, T, 3, H, W]")
        T, _, H, W = pixels.shape[1:]
        slot = self._n % self.slots
        if self._done[slot] is not None:
            self._done[slot].synchronize()                      # the slot's previous copy must have landed before reuse
        if self._key[slot] != (T, H, W):
            bound = ops.jpeg_out_bound(T, H, W)
            if bound == 0:
                raise ValueError(f"JpegFrameDownloader: cannot encode {T} frames of {H} x {W} (H and W multiples of 8, "
                                 "at most RTV_FRAMES_MAX frames per block)")
            self._arena[slot] = torch.empty(ops.jpeg_arena_bytes(T, H, W), dtype=torch.uint8, device=self.device)
            self._dev[slot] = torch.empty(bound, dtype=torch.uint8, device=self.device)
            self._offs[slot] = torch.zeros(T + 1, dtype=torch.int64, device=self.device)
            self._host_offs[slot] = torch.zeros(T + 1, dtype=torch.int64).pin_memory()
            self._key[slot] = (T, H, W)
        n = min(self._estimate(T, H, W), self._dev[slot].numel())
        if self._host[slot] is None or self._host[slot].numel() < n:
            self._host[slot] = torch.empty(n, dtype=torch.uint8, pin_memory=True)
        if event is None:
            event = torch.cuda.Event()
            event.record(torch.cuda.current_stream(self.device))
        self.stream.wait_event(event)                           # :981 download_stream.wait_event(event)
        with torch.cuda.stream(self.stream):
            src = pixels[0].float().contiguous()
            src.record_stream(self.stream)
            ops.jpeg_encode(src, self.quality, out=self._dev[slot], offsets=self._offs[slot], arena=self._arena[slot])
            self._host_offs[slot].copy_(self._offs[slot], non_blocking=True)
            self._host[slot][:n].copy_(self._dev[slot][:n], non_blocking=True)
            done = torch.cuda.Event()
            done.record(self.stream)
        self._done[slot], self._copied[slot], self._frame_ids[slot] = done, n, list(frame_ids)
        self._n += 1
        return self._n - 1

    def fetch(self, ticket):
        if not (self._n - self.slots <= ticket < self._n) or ticket < 0:
            raise KeyError(f"ticket {ticket} is no longer (or not yet) held; {self.slots} slots")
        slot = ticket % self.slots
        self._done[slot].synchronize()
        offs = self._host_offs[slot].tolist()
        total, have = offs[-1], self._copied[slot]
        self._largest = max(self._largest, total)
        if total > have:                                        # the estimate fell short: the rest, into a buffer that holds it all
            if self._host[slot].numel() < total:
                grown = torch.empty((total * 5 + 3) // 4, dtype=torch.uint8, pin_memory=True)
                grown[:have].copy_(self._host[slot][:have])
                self._host[slot] = grown
            with torch.cuda.stream(self.stream):
                self._host[slot][have:total].copy_(self._dev[slot][have:total], non_blocking=True)
                self._done[slot].record(self.stream)
            self._done[slot].synchronize()
            self._copied[slot] = total
            self.topups += 1
        files = memoryview(self._host[slot].numpy())
        return [files[a:b] for a, b in zip(offs[:-1], offs[1:])]

    def frame_ids(self, ticket):
        return self._frame_ids[ticket % self.slots]


class FrameUploader:
    """`push(frame)` copies one uint8 [H, W, 3] frame (CPU torch / numpy, or a CUDA tensor) into a pinned ring slot and on into
    the device ring slot of the same number on the upload stream, and returns a ticket; `gather(tickets, size)` makes the current
    stream wait for those uploads and returns the frames as float16 [3, T, h, w] in [-1, 1] from one kernel launch.  A ticket is
    valid until its slot is reused `slots` pushes later, or until a frame of another size reallocates the rings.

    `push_jpeg(file)` is `push` for a JPEG file (bytes / bytearray / memoryview): the host parses the marker segments (ValueError
    for a file the decoder refuses, before anything is queued), descriptor and file go into a pinned slot of a second ring, and
    the upload stream copies them up and decodes them straight into the rgb8 ring slot (one rtv_jpeg_decode call).  The ticket
    is of the same kind, raw and JPEG pushes may alternate, `gather` is the same.  `status(ticket)` waits for that upload only and
    returns the frame's status word (0 = clean; a raw frame's is 0).  A file slot holds the frame's raw size plus 1 KiB: a file
    larger than its own pixels is refused."""

    def __init__(self, device="cuda", slots=32):
        if slots < 1:
            raise ValueError("slots must be >= 1")
        self.device = torch.device(device)
        self.stream = torch.cuda.Stream(device=self.device)     # release_server.py:88-90 upload_stream
        self.slots = slots
        self._host = self._dev = None                           # uint8 [slots, H, W, 3]: pinned ring, device ring
        self._done = [None] * slots                             # upload of the slot has landed (upload stream)
        self._read = [None] * slots                             # last gather that reads the slot (its stream)
        self._n = 0
        self._first = 0                                         # oldest ticket of the present rings
        self._jhost = self._jdev = None                         # uint8 [slots, cap]: descriptor plus file, pinned ring / device ring
        self._jshape = None                                     # the frame size the file rings are sized for
        self._jarena = None                                     # the decoder's scratch: calls are serial on the upload stream
        self._jstatus = self._jstatus_host = None               # int32 [slots]: device, pinned
        self._is_jpeg = [False] * slots

    def _held(self, ticket):
        return max(self._first, self._n - self.slots) <= ticket < self._n

    def _rings(self, shape):
        if self._dev is None or tuple(shape) != tuple(self._dev.shape[1:]):
            # first frame, or the camera changed resolution: new rings, the old tickets are gone.  Copies in flight keep the old
            # rings alive (pinned memory and record_stream defer the reuse of their memory), so nothing waits here.
            self._host = torch.empty((self.slots,) + tuple(shape), dtype=torch.uint8, pin_memory=True)
            self._dev = torch.empty((self.slots,) + tuple(shape), dtype=torch.uint8, device=self.device)
            self._dev.record_stream(self.stream)
            self._done, self._read = [None] * self.slots, [None] * self.slots
            self._first = self._n
            self._jshape = None                                 # the file rings go with them: their slots' events are gone too

    def push(self, frame):
        if not torch.is_tensor(frame):
            frame = torch.from_numpy(frame)
        if frame.dtype != torch.uint8 or frame.dim() != 3 or frame.shape[2] != 3:
            raise ValueError("FrameUploader.push expects a uint8 [H, W, 3] frame")
        self._rings(frame.shape)
        slot = self._n % self.slots
        self._is_jpeg[slot] = False
        if self._read[slot] is not None:
            self.stream.wait_event(self._read[slot])            # a gather may still read the slot the upload overwrites
        if frame.is_cuda:
            produced = torch.cuda.Event()
            produced.record(torch.cuda.current_stream(self.device))
            self.stream.wait_event(produced)
            with torch.cuda.stream(self.stream):
                self._dev[slot].copy_(frame, non_blocking=True)
                frame.record_stream(self.stream)
        else:
            if self._done[slot] is not None:
                self._done[slot].synchronize()                  # the pinned slot's previous upload must have landed before reuse
            self._host[slot].copy_(frame)
            with torch.cuda.stream(self.stream):
                self._dev[slot].copy_(self._host[slot], non_blocking=True)
        done = torch.cuda.Event()
        done.record(self.stream)
        self._done[slot] = done
        self._n += 1
        return self._n - 1

    def push_jpeg(self, data):
        import ctypes
        if isinstance(data, (bytearray, memoryview)):
            data = bytes(data)
        if not isinstance(data, bytes):
            raise TypeError("FrameUploader.push_jpeg expects a JPEG file as bytes, bytearray or memoryview")
        info = ops.jpeg_parse(data)                             # ValueError for a refusal: nothing has been queued
        shape = (info.H, info.W, 3)
        cap = (ops.JPEG_DESC_BYTES + info.H * info.W * 3 + 1024 + 15) // 16 * 16
        n = ops.JPEG_DESC_BYTES + len(data)
        if n > cap:
            raise ValueError(f"FrameUploader.push_jpeg: a file of {len(data)} bytes for {info.H} x {info.W} pixels is larger than "
                             "its own raw pixels; decode it on the host and push the pixels")
        self._rings(shape)
        if self._jshape != shape:
            self._jhost = torch.empty((self.slots, cap), dtype=torch.uint8, pin_memory=True)
            self._jdev = torch.empty((self.slots, cap), dtype=torch.uint8, device=self.device)
            self._jdev.record_stream(self.stream)
            self._jshape = shape
        if self._jstatus is None:
            self._jstatus = torch.zeros(self.slots, dtype=torch.int32, device=self.device)
            self._jstatus.record_stream(self.stream)
            self._jstatus_host = torch.zeros(self.slots, dtype=torch.int32).pin_memory()
        need = ops.jpeg_decode_arena_bytes([info])
        if self._jarena is None or self._jarena.numel() < need:
            self._jarena = torch.empty(need, dtype=torch.uint8, device=self.device)
            self._jarena.record_stream(self.stream)
        slot = self._n % self.slots
        if self._read[slot] is not None:
            self.stream.wait_event(self._read[slot])            # a gather may still read the slot the decode overwrites
        if self._done[slot] is not None:
            self._done[slot].synchronize()                      # the pinned slot's previous upload must have landed before reuse
        at = self._jhost[slot].data_ptr()
        ctypes.memmove(at, ctypes.byref(info.desc), ops.JPEG_DESC_BYTES)
        ctypes.memmove(at + ops.JPEG_DESC_BYTES, data, len(data))
        with torch.cuda.stream(self.stream):
            self._jdev[slot, :n].copy_(self._jhost[slot, :n], non_blocking=True)
            ops.jpeg_decode_frames([info], [self._jdev[slot]], [self._dev[slot]], self._jstatus[slot:slot + 1], self._jarena)
            self._jstatus_host[slot:slot + 1].copy_(self._jstatus[slot:slot + 1], non_blocking=True)
        done = torch.cuda.Event()
        done.record(self.stream)
        self._done[slot], self._is_jpeg[slot] = done, True
        self._n += 1
        return self._n - 1

    def status(self, ticket):
        if not self._held(int(ticket)):
            raise KeyError(f"ticket {ticket} is no longer (or not yet) held; {self.slots} slots")
        slot = int(ticket) % self.slots
        if not self._is_jpeg[slot]:
            return 0
        self._done[slot].synchronize()
        return int(self._jstatus_host[slot])

    def gather(self, tickets, size):
        tickets = [int(t) for t in tickets]
        for t in tickets:
            if not self._held(t):
                raise KeyError(f"ticket {t} is no longer (or not yet) held; {self.slots} slots")
        if not tickets:
            raise ValueError("FrameUploader.gather needs at least one ticket")
        slots = [t % self.slots for t in tickets]
        current = torch.cuda.current_stream(self.device)
        for slot in set(slots):
            current.wait_event(self._done[slot])
        self._dev.record_stream(current)
        out = ops.frames_from_rgb8(self._dev, size, slots=slots)
        read = torch.cuda.Event()
        read.record(current)
        for slot in set(slots):
            self._read[slot] = read
        return out
