"""The scratch of the 128-channel 15x15 search kernels, read from the kernel descriptors of the gfx950 code object inside the built
library (no GPU needed): the streamed heads loop (csrc/azg_conv.h heads_full_stream) is what keeps them below the 64-channel persistent
kernel, whose spill is the unrolled heads' 113 weight fragments.  The bound is the issue's: below 2176 B/lane, the 64-channel persistent
kernel's figure, reported next to the stand-alone 128-channel tower's 340 B/lane (profiles/gobang128_kernel_resources.txt)."""
import struct

from alphazero_general_amd import build as B

TOWER = '_ZN3azg8k_tower2ILi15ELi15ELi1ELi%dELi3ENS_%sELi1EEEvNS_11TowerParamsEPKsT4_'
SEARCH, ARENA, NOSEARCH = '10SearchWideINS_2GBELi1ELb1EE', '15SearchWideArenaINS_2GBELi1EE', '8NoSearch'


def _code_object(path):
    d = open(path, 'rb').read()
    i = d.find(b'__CLANG_OFFLOAD_BUNDLE__')
    assert i >= 0, 'no offload bundle in the library'
    n, = struct.unpack_from('<Q', d, i + 24)
    o = i + 32
    for _ in range(n):
        off, size, tl = struct.unpack_from('<QQQ', d, o)
        triple = d[o + 24:o + 24 + tl]
        o += 24 + tl
        if b'gfx950' in triple:
            return d[i + off:i + off + size]
    raise AssertionError('no gfx950 code object in the library')


def _scratch_bytes(elf):
    """kernel name -> private_segment_fixed_size (bytes per lane), from the 64-byte kernel descriptors `<kernel>.kd`"""
    assert elf[:4] == b'\x7fELF' and elf[4] == 2
    shoff, = struct.unpack_from('<Q', elf, 0x28)
    shentsize, shnum = struct.unpack_from('<HH', elf, 0x3A)
    secs = [struct.unpack_from('<IIQQQQIIQQ', elf, shoff + k * shentsize) for k in range(shnum)]
    out = {}
    for (_, typ, _, _, off, size, link, _, _, entsize) in secs:
        if typ != 2:                                         # SHT_SYMTAB
            continue
        stroff = secs[link][4]
        for k in range(size // entsize):
            name, _, _, shndx, value, _ = struct.unpack_from('<IBBHQQ', elf, off + k * entsize)
            end = elf.index(b'\0', stroff + name)
            sym = elf[stroff + name:end].decode()
            if sym.endswith('.kd') and 0 < shndx < shnum:
                s = secs[shndx]
                kd = s[4] + (value - s[3])
                out[sym[:-3]] = struct.unpack_from('<II', elf, kd)[1]
    return out


def test_gb128_search_kernels_scratch_below_the_unrolled_heads():
    scratch = _scratch_bytes(_code_object(B.out_path()))
    tower, wide64 = scratch[TOWER % (128, NOSEARCH)], scratch[TOWER % (64, SEARCH)]
    new = {k: scratch[TOWER % (128, k)] for k in (SEARCH, ARENA)}
    print('ScratchSize [B/lane]: stand-alone 128-channel tower %d, 64-channel persistent kernel %d, new %s' % (tower, wide64, new))
    assert tower == 340 and wide64 == 2176                   # the two figures of the issue: these kernels are not changed here
    for k, v in new.items():
        assert v < 2176, (k, v)
