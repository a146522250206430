"""What the filter banks' GPU tests share (test_gpu_channelizer.py, test_gpu_combine.py): the handle and its buffers, a
kernel's tile constant, comparison by bits, and buffers that hold a canary wherever a call may not write."""
import os
import re

import numpy as np

from wifirx import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CANARY = 0xA5


def tile(header, macro):
    """the value of a #define in a header under csrc/"""
    txt = open(os.path.join(ROOT, "gnuradio-wifi-imagetransfer_amd", "csrc", header)).read()
    return int(re.search(r"#define\s+%s\s+(\d+)" % macro, txt).group(1))


def open_rx():
    """the body of a module's rx fixture"""
    r = capi.WifiRx(max_sym=1, device=0)
    yield r
    r.close()


def alloc_bufs(rx, **nbytes):
    """the body of a module's bufs fixture: one device buffer per keyword"""
    b = {k: rx.alloc(n) for k, n in nbytes.items()}
    yield b
    for d in b.values():
        d.free()


def bits_of(a):
    return np.ascontiguousarray(a).view(np.uint8).reshape(-1)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits_of(a), bits_of(b))


def fill(buf):
    """the canary in every byte of a device buffer; returns what was uploaded"""
    raw = np.full(buf.nbytes, CANARY, np.uint8)
    buf.upload(raw)
    return raw


def download_fenced(buf, spans, what):
    """every byte of a buffer that was filled before the call; outside the (first byte, bytes) spans the canary still stands"""
    raw = buf.download(np.uint8, buf.nbytes)
    mask = np.ones(buf.nbytes, bool)
    for a, n in spans:
        mask[a:a + n] = False
    assert (raw[mask] == CANARY).all(), "wrote outside " + what
    return raw
