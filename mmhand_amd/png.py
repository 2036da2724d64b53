"""PNG files decoded on the device (opt-in: `HandFolderLoader(device_png=True)`, --device_png, MMH_DEVICE_PNG=1).

The host walks the container - signature, IHDR, chunk CRCs, the IDAT payloads joined in file order (`parse_png`) - and uploads
the zlib streams of a whole batch as one buffer; `mmh_png_decode_batch` (csrc/png_decode.hip) inflates, checks the Adler-32,
unfilters and writes uint8 [N,H,W,3] in cv2.imread's B,G,R order, the batch `mmh_decode_inputs` consumes.  Only what the
prepared RHD / STB directories hold goes to the device: 8-bit, colour type 2 (RGB), non-interlaced, all of one size.  Any
other file (16-bit, palette, grey, alpha, Adam7, another size, a container error) and any image whose device status is not 0
is decoded by PIL exactly as `data._read_bgr` does and copied into its slot; the caller is told which and why.  A file PIL
rejects too raises, as it does on the default path.

The other direction (opt-in: `python -m mmhand_amd.aug ... --device_png`): `PngBatchEncoder` hands a uint8 [N,H,W,3] device
batch to `mmh_png_encode_batch` (csrc/png_encode.hip: row filters + Huffman-only DEFLATE, one zlib stream per image), fetches
the streams and wraps each in the container (`write_png`: signature, IHDR, one IDAT, IEND, CRCs by zlib.crc32).  An image whose
device status is not 0 is encoded by PIL from the same pixels and reported, as on the decode side."""
import ctypes as C
import io
import struct
import zlib

import numpy as np
import torch

from . import lib as L

SIGNATURE = b"\x89PNG\r\n\x1a\n"

# the enum of include/mmhand_hip.h
STATUS = {0: "ok", 1: "zlib header", 2: "preset dictionary", 3: "truncated", 4: "block type 3", 5: "stored LEN != ~NLEN",
          6: "over-subscribed code", 7: "incomplete code", 8: "repeat without previous length", 9: "too many code lengths",
          10: "no end-of-block code", 11: "invalid length / distance symbol", 12: "unassigned code", 13: "distance too far back",
          14: "output too long", 15: "output too short", 16: "data after the trailer", 17: "Adler-32 mismatch",
          18: "filter type above 4", 19: "step bound", 20: "stream range"}


def parse_png(data):
    """(width, height, bit_depth, colour_type, interlace, idat) of a PNG file's bytes; idat = the IDAT payloads concatenated in
    file order (one zlib stream).  ValueError on a bad signature, a chunk that runs past the end, a CRC mismatch, a missing
    or misplaced IHDR, no IDAT or no IEND."""
    mv = memoryview(data)
    if len(mv) < 8 or bytes(mv[:8]) != SIGNATURE:
        raise ValueError("not a PNG: bad signature")
    pos, ihdr, idat, end = 8, None, [], False
    while pos < len(mv):
        if pos + 8 > len(mv):
            raise ValueError("PNG: truncated chunk header")
        n, typ = struct.unpack_from(">I4s", mv, pos)
        if pos + 12 + n > len(mv):
            raise ValueError(f"PNG: chunk {typ!r} runs past the end of the file")
        body = mv[pos + 8:pos + 8 + n]
        if zlib.crc32(body, zlib.crc32(typ)) != struct.unpack_from(">I", mv, pos + 8 + n)[0]:
            raise ValueError(f"PNG: CRC mismatch in chunk {typ!r}")
        if ihdr is None:
            if typ != b"IHDR" or n != 13:
                raise ValueError("PNG: the first chunk is not a 13-byte IHDR")
            ihdr = struct.unpack(">IIBBBBB", body)
        elif typ == b"IHDR":
            raise ValueError("PNG: second IHDR")
        elif typ == b"IDAT":
            idat.append(body)
        elif typ == b"IEND":
            end = True
            break
        pos += 12 + n
    if ihdr is None or not idat or not end:
        raise ValueError("PNG: missing IHDR, IDAT or IEND")
    w, h, depth, colour, comp, flt, interlace = ihdr
    if w == 0 or h == 0 or comp != 0 or flt != 0:
        raise ValueError("PNG: invalid IHDR")
    return w, h, depth, colour, interlace, b"".join(idat)


def pil_decode(data, bgr=True):
    """`data._read_bgr` on a file's bytes: uint8 [H,W,3]"""
    from PIL import Image
    with Image.open(io.BytesIO(data)) as im:
        rgb = np.asarray(im.convert("RGB"), dtype=np.uint8)
    return np.ascontiguousarray(rgb[:, :, ::-1]) if bgr else np.ascontiguousarray(rgb)


def _chunk(typ, body):
    return struct.pack(">I", len(body)) + typ + body + struct.pack(">I", zlib.crc32(body, zlib.crc32(typ)))


def write_png(w, h, idat):
    """the file around one zlib stream: signature, IHDR (8-bit, colour type 2, no interlace), one IDAT, IEND"""
    return (SIGNATURE + _chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 0)) + _chunk(b"IDAT", bytes(idat))
            + _chunk(b"IEND", b""))


def pil_encode(rgb):
    """PIL's default PNG of uint8 [H,W,3] R,G,B pixels (what aug.py writes without --device_png)"""
    from PIL import Image
    b = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(rgb)).save(b, format="PNG")
    return b.getvalue()


ENC_STATUS = {0: "ok", 1: "stream longer than its slot"}


def _pinned(n, dtype):
    t = torch.empty(n, dtype=dtype)
    return t.pin_memory() if torch.cuda.is_available() else t


class PngBatchDecoder:
    """One set of buffers - pinned stream / offsets / status on the host, stream / offsets / scratch / output / status on the
    device - for batches of up to `capacity` images; reused batch after batch (it grows only when a batch needs more).  The
    output of `decode` is a view of this set's output buffer: valid until the set decodes again."""

    def __init__(self, device):
        self.device = torch.device(device)
        self.cap = self.shape = None
        self.stream_h = self.stream_d = None
        self.done = None

    def _reserve(self, n, h, w, nbytes):
        if self.cap is None or n > self.cap or (h, w) != self.shape:
            self.cap, self.shape = n, (h, w)
            self.off_h, self.st_h = _pinned(n + 1, torch.int64), _pinned(n, torch.int32)
            self.off_d = torch.empty(n + 1, dtype=torch.int64, device=self.device)
            self.st_d = torch.empty(n, dtype=torch.int32, device=self.device)
            self.scratch = torch.empty(n * h * (1 + 3 * w), dtype=torch.uint8, device=self.device)
            self.out = torch.empty((n, h, w, 3), dtype=torch.uint8, device=self.device)
        if self.stream_h is None or nbytes > self.stream_h.numel():
            room = max(nbytes + nbytes // 4, n * (h * (1 + 3 * w) // 2 + 64))
            self.stream_h = _pinned(room, torch.uint8)
            self.stream_d = torch.empty(room, dtype=torch.uint8, device=self.device)

    def pack(self, files):
        """host half: parse every file, lay the device-eligible streams into the pinned buffer.  Returns the plan `launch`
        takes: (n, h, w, nbytes, fallbacks, files) with fallbacks = {index: (reason, pixels decoded by PIL)}."""
        n = len(files)
        parsed, fallbacks, shape = [None] * n, {}, None
        for i, f in enumerate(files):
            try:
                w, h, depth, colour, interlace, idat = parse_png(f)
            except ValueError as e:
                fallbacks[i] = (f"container: {e}", None)
                continue
            if depth != 8 or colour != 2 or interlace != 0:
                fallbacks[i] = (f"format: bit depth {depth}, colour type {colour}, interlace {interlace}", None)
                continue
            if shape is None:
                shape = (h, w)
            if (h, w) != shape:
                fallbacks[i] = (f"size: {h}x{w} in a batch of {shape[0]}x{shape[1]}", None)
                continue
            parsed[i] = idat
        if self.done is not None:
            self.done.synchronize()             # this set's previous upload and decode have left the pinned buffers
        for i in fallbacks:                     # a file PIL rejects as well raises here, as on the default path
            fallbacks[i] = (fallbacks[i][0], pil_decode(files[i], bgr=True))
        if shape is None:                       # nothing for the device: the batch's size is PIL's
            shape = next(iter(fallbacks.values()))[1].shape[:2] if fallbacks else (1, 1)
        nbytes = sum(len(p) for p in parsed if p is not None)
        self._reserve(n, shape[0], shape[1], nbytes)
        buf, off, pos = self.stream_h.numpy(), self.off_h.numpy(), 0
        for i, p in enumerate(parsed):
            off[i] = pos
            if p is not None:
                buf[pos:pos + len(p)] = np.frombuffer(p, dtype=np.uint8)
                pos += len(p)
        off[n:] = pos
        return n, shape[0], shape[1], nbytes, fallbacks, files

    def launch(self, plan, bgr=True, stream=None):
        """device half: upload, decode, fetch the statuses, patch the fallback slots.  Returns (out [n,H,W,3] uint8 view,
        [(index, reason)])."""
        n, h, w, nbytes, fallbacks, files = plan
        if n == 0:
            return torch.empty((0, h, w, 3), dtype=torch.uint8, device=self.device), []
        stream = stream or torch.cuda.current_stream(self.device)
        with torch.cuda.stream(stream):
            self.stream_d[:nbytes].copy_(self.stream_h[:nbytes], non_blocking=True)
            self.off_d[:n + 1].copy_(self.off_h[:n + 1], non_blocking=True)
            L.call("mmh_png_decode_batch", C.c_void_p(self.stream_d.data_ptr()), nbytes, C.c_void_p(self.off_d.data_ptr()), n,
                   h, w, C.c_void_p(self.scratch.data_ptr()), C.c_void_p(self.out.data_ptr()),
                   C.c_void_p(self.st_d.data_ptr()), int(bool(bgr)), C.c_void_p(stream.cuda_stream))
            self.st_h[:n].copy_(self.st_d[:n], non_blocking=True)
            self.done = torch.cuda.Event()
            self.done.record(stream)
            self.done.synchronize()             # the statuses decide what the caller may read
            status = self.st_h[:n].numpy()
            report = []
            for i in range(n):
                if i in fallbacks:
                    reason, px = fallbacks[i]
                elif status[i] != 0:
                    reason, px = f"device status {int(status[i])}: {STATUS.get(int(status[i]), '?')}", None
                else:
                    continue
                report.append((i, reason))
                fallbacks[i] = (reason, px)
            for i, _ in report:
                px = fallbacks[i][1]
                if px is None:
                    px = pil_decode(files[i], bgr=True)
                if not bgr:
                    px = np.ascontiguousarray(px[:, :, ::-1])
                if px.shape != (h, w, 3):
                    raise ValueError(f"PNG batch: image {i} is {px.shape[0]}x{px.shape[1]}, the batch {h}x{w}")
                self.out[i].copy_(torch.from_numpy(px))
        return self.out[:n], report

    def decode(self, files, bgr=True, stream=None):
        return self.launch(self.pack(files), bgr=bgr, stream=stream)


def decode_png_batch(files, device, bgr=True, stream=None):
    """files: the bytes of N PNG files of one size -> (uint8 [N,H,W,3] on `device`, B,G,R per pixel if bgr else R,G,B;
    [(index, reason)] for the files that went through PIL instead of the device)."""
    return PngBatchDecoder(device).decode(list(files), bgr=bgr, stream=stream)


class PngBatchEncoder:
    """One set of buffers - scratch / stream slots / lengths / status on the device, pinned lengths / status / streams on the
    host - for batches of up to `capacity` images of one size; reused batch after batch (it grows only when a batch needs
    more).  `launch` enqueues the encode and the copy of lengths and statuses and returns at once; `fetch` waits for them,
    copies each stream's bytes (not the slots' slack) and builds the files - so a caller may enqueue other work in between.
    One plan at a time: the buffers belong to the launched batch until it is fetched, and a second `launch` before raises.
    slot_bytes: a smaller slot than mmh_png_encode_slot_bytes (tests; an image that does not fit goes through PIL)."""

    def __init__(self, device, slot_bytes=None):
        self.device = torch.empty(0, device=device).device          # "cuda" -> the current device, with its index
        self.cap = self.shape = None
        self.slot_override = slot_bytes
        self.done = None
        self.in_flight = False

    def _reserve(self, n, h, w):
        if self.cap is None or n > self.cap or (h, w) != self.shape:
            lib = L.load()
            self.cap, self.shape = n, (h, w)
            self.slot = int(self.slot_override or lib.mmh_png_encode_slot_bytes(h, w))
            if self.slot < 8:
                raise ValueError(f"PNG batch: cannot encode images of {h}x{w}")
            self.scratch = torch.empty(int(lib.mmh_png_encode_scratch_bytes(n, h, w)), dtype=torch.uint8, device=self.device)
            self.slots_d = torch.empty((n, self.slot), dtype=torch.uint8, device=self.device)
            self.len_d = torch.empty(n, dtype=torch.int64, device=self.device)
            self.st_d = torch.empty(n, dtype=torch.int32, device=self.device)
            self.len_h, self.st_h = _pinned(n, torch.int64), _pinned(n, torch.int32)
            self.slots_h = _pinned(n * self.slot, torch.uint8).view(n, self.slot)

    def launch(self, pixels, bgr=False, stream=None):
        """device half: pixels uint8 [N,H,W,3] on the device (kept alive by the returned plan until `fetch`)"""
        if pixels.dtype != torch.uint8 or pixels.dim() != 4 or pixels.shape[3] != 3 or pixels.device != self.device:
            raise ValueError("PNG batch: expected a uint8 [N,H,W,3] tensor on the encoder's device")
        pixels = pixels.contiguous()
        n, h, w, _ = pixels.shape
        if self.in_flight:
            raise RuntimeError("PngBatchEncoder.launch: the previous batch has not been fetched; its buffers are still in use")
        if n == 0:
            return pixels, bool(bgr), None
        if self.done is not None:
            self.done.synchronize()             # the previous batch has left this set's buffers
        self._reserve(n, h, w)
        stream = stream or torch.cuda.current_stream(self.device)
        with torch.cuda.stream(stream):
            L.call("mmh_png_encode_batch", C.c_void_p(pixels.data_ptr()), n, h, w, int(bool(bgr)),
                   C.c_void_p(self.scratch.data_ptr()), C.c_void_p(self.slots_d.data_ptr()), self.slot,
                   C.c_void_p(self.len_d.data_ptr()), C.c_void_p(self.st_d.data_ptr()), C.c_void_p(stream.cuda_stream))
            self.len_h[:n].copy_(self.len_d[:n], non_blocking=True)
            self.st_h[:n].copy_(self.st_d[:n], non_blocking=True)
            self.done = torch.cuda.Event()
            self.done.record(stream)
        self.in_flight = True
        return pixels, bool(bgr), stream

    def fetch(self, plan):
        """host half -> (list of N files' bytes, [(index, reason)] for the images PIL encoded instead)"""
        pixels, bgr, stream = plan
        n, h, w, _ = pixels.shape
        if n == 0:
            return [], []
        if not self.in_flight:
            raise RuntimeError("PngBatchEncoder.fetch: no launched batch to fetch")
        self.done.synchronize()
        lengths, status = self.len_h[:n].numpy().copy(), self.st_h[:n].numpy().copy()
        with torch.cuda.stream(stream):
            for i in range(n):
                if status[i] == 0:
                    k = int(lengths[i])
                    self.slots_h[i, :k].copy_(self.slots_d[i, :k], non_blocking=True)
            self.done = torch.cuda.Event()
            self.done.record(stream)
        self.done.synchronize()
        self.in_flight = False
        files, report = [], []
        for i in range(n):
            if status[i] == 0:
                files.append(write_png(w, h, self.slots_h[i, :int(lengths[i])].numpy().tobytes()))
                continue
            report.append((i, f"device status {int(status[i])}: {ENC_STATUS.get(int(status[i]), '?')}"))
            px = pixels[i].cpu().numpy()
            files.append(pil_encode(px[:, :, ::-1] if bgr else px))
        return files, report

    def encode(self, pixels, bgr=False, stream=None):
        return self.fetch(self.launch(pixels, bgr=bgr, stream=stream))


def encode_png_batch(pixels, bgr=False, stream=None):
    """pixels: uint8 [N,H,W,3] on a device, B,G,R per pixel if bgr else R,G,B -> (the bytes of N PNG files, [(index, reason)]
    for the images that went through PIL instead of the device)"""
    return PngBatchEncoder(pixels.device).encode(pixels, bgr=bgr, stream=stream)
