"""The compressor over groups and the BGZF writer's tiles through the entry points that need no GPU:
fc2_deflate_launch_groups and fc2_gpu_bgzf_tiles refuse what cannot be groups or tiles before they touch a
device, and fc2_deflate_group_tiles counts the tiles of a launch."""
import ctypes

from find_circ2_amd import _native as N

E_PARAM = -1


def test_launch_groups_refuses_before_the_device():
    L = N.lib()
    buf = (ctypes.c_uint8 * 64)()
    p = ctypes.addressof(buf)
    for group, tile, hist, level in [(0, 64, 0, 1), (100, 0, 0, 1), (100, 65537, 0, 1), (100, 64, 32769, 1),
                                     (100, 32769, 32768, 1), (100, 64, 0, 0), (100, 64, 0, 3)]:
        assert L.fc2_deflate_launch_groups(p, 8, group, tile, hist, p, 65537 + 16, p, p, p, None, level) == E_PARAM
    assert L.fc2_deflate_launch_groups(p, 8, 100, 64, 0, p, 64, p, p, p, None, 1) == E_PARAM          # the stride
    assert L.fc2_deflate_launch_groups(p, 0, 100, 64, 0, p, 80, p, p, p, None, 1) == 0                # nothing to do
    assert L.fc2_deflate_group_tiles(217, 100, 64) == 5 and L.fc2_deflate_group_tiles(200, 100, 25) == 8
    assert L.fc2_deflate_group_tiles(217, 0, 64) == 0 == L.fc2_deflate_group_tiles(217, 100, 0)


def test_gpu_bgzf_tiles_refuses_before_the_device():
    L = N.lib()
    n = ctypes.c_uint64(7)
    out = (ctypes.c_uint8 * 128)()
    src = ctypes.create_string_buffer(b"abc", 3)
    for block, tile, hist, level in [(0xff00, 0xff00 // 17, 0, 1),        # 17 tiles a block
                                     (0xff00, 16320, 32769, 1), (0xff00, 40000, 32768, 1), (0xff00, 16320, 0, 3),
                                     (0xff01, 16320, 0, 1), (0, 16, 0, 1)]:
        assert L.fc2_gpu_bgzf_tiles(0, src, 3, block, 4, tile, hist, level, out, 128, ctypes.byref(n)) == E_PARAM
    assert L.fc2_gpu_bgzf_tiles(0, src, 0, 0xff00, 4, 16320, 32768, 1, out, 128, ctypes.byref(n)) == 0 and n.value == 0
    assert L.fc2_gpu_bgzf_tiles_bound(3, 0xff00, 0) == L.fc2_gpu_bgzf_bound(3, 0xff00) == L.fc2_gpu_bgzf_tiles_bound(3, 0xff00, 0xff00)
    assert L.fc2_gpu_bgzf_tiles_bound(0xff00, 0xff00, 0xff00 // 16) == 0xff00 + 26 + 256
    assert L.fc2_gpu_bgzf_tiles_bound(3, 0xff01, 16) == 0
