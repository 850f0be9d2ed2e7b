// An lzip file, walked: its members found in bytes that come in order, cut anywhere (the format: lzip_member.h).  ONE walker
// for the host reader (host/lzip.cpp), which pulls bytes until a member is whole, and for the device decoder's round
// (lzip_decode.hip), which is pushed bytes and takes whole members.  Peek, then take, as xz::Walker.
// A member's sizes lie at its END, so the walker searches and decodes nothing.  The member that starts at s ends at q when
//   p[q, q + 6) is a legal header (magic, version 1, legal DS) -- or q is the end of the bytes and no more will come --,
//   le64(p + q - 8) == q - s   (the trailer's member_size), and
//   q - s >= 6 + 5 + 20.
// A magic that fails the member_size test lies inside compressed data: it is passed over, the search goes on, and nothing
// else is guessed.  (A false positive needs a chance 64-bit match -- and the decode must still end with the marker at that
// trailer, with its CRC32.)  The search keeps a cursor (`searched`, a file offset): what one peek has searched the next does
// not search again, so bytes fed one at a time cost no more than bytes fed at once.
// At the file's end a member that no q closes is truncated -- unless its member_size closes on a q in front of the end: then
// what lies behind q is no member: trailing data (the first bytes of a header are a member's, a truncated one's).  Host only.
#pragma once
#include <cstring>
#include <string>

#include "lzip_member.h"

namespace slimm {
namespace lzip {

inline std::string place_text(uint64_t at) { return "member at byte " + std::to_string(at); }

struct Walker {
    uint64_t members = 0;    // taken so far
    uint64_t searched = 0;   // the member at hand has no end in front of this file offset (0: not searched)

    // More: the bytes end inside what stands here -- `want` of them are needed at least, `status` is the verdict if the input
    // is over.  Error: `status`.  MayEnd: no byte is left, and the file may end here
    enum Kind : uint8_t { More, Error, MayEnd, MemberItem };
    struct Item {
        Kind kind = More;
        uint64_t at = 0;          // the member's file offset (kTrailing: that of the bytes that are none)
        uint32_t status = kOk;
        uint64_t want = 0;
        uint64_t bytes = 0;       // MemberItem: member_size -- what take() moves past
        uint32_t dict_size = 0;
        Trailer trailer{};
        uint64_t searched = 0;    // the cursor behind this peek (take keeps it)
        std::string where() const { return place_text(at); }
        std::string words() const { return status == kTrailing ? "at byte " + std::to_string(at) + ": " + status_text(status) : where() + ": " + status_text(status); }
        Item& more(uint64_t n, uint32_t verdict = kRanOut) { return kind = More, want = n, status = verdict, *this; }
        Item& error(uint32_t cause) { return kind = Error, status = cause, *this; }
    };

    // does a legal header stand at p[0, 6)?
    static bool header_at(const uint8_t* p) {
        uint32_t d = 0;
        return member_header(p, &d) == kOk;
    }

    // what stands at p[0, avail), file offset `base`, where a member starts; at_end: no byte will follow these
    Item peek(const uint8_t* p, uint64_t avail, uint64_t base, bool at_end) const {
        Item it;
        it.at = base;
        it.searched = searched;
        if (avail == 0 && members > 0) return it.kind = MayEnd, it;
        if (avail < kHeaderBytes) {
            if (magic_prefix(p, avail) && (avail < 5u || p[4] == 1u)) return it.more(kHeaderBytes);
            return members > 0 ? it.error(kTrailing) : it.more(kHeaderBytes, kNoMember);
        }
        const uint32_t hs = member_header(p, &it.dict_size);
        if (hs != kOk) return it.error(hs == kNoMember && members > 0 ? kTrailing : hs);
        // the search, from the cursor on: every q whose header's six bytes are at hand
        uint64_t q = kMemberMin;
        if (searched > base + q) q = searched - base;
        for (; q + kHeaderBytes <= avail; ++q) {
            const void* hit = memchr(p + q, 'L', avail - kHeaderBytes + 1u - q);
            if (!hit) {
                q = avail - kHeaderBytes + 1u;
                break;
            }
            q = static_cast<uint64_t>(static_cast<const uint8_t*>(hit) - p);
            if (xz::le64(p + q - 8u) == q && header_at(p + q)) return member(p, q, it);
        }
        it.searched = base + q;
        if (!at_end) return it.more(avail + 1u);
        if (avail >= kMemberMin && xz::le64(p + avail - 8u) == avail) return member(p, avail, it);
        // no end: is there a member_size that closes in front of the end, with no member behind it?
        // (what is left of a header that the file ends in starts a member all the same: that one is truncated, not this)
        for (uint64_t k = kMemberMin; k < avail; ++k)
            if (xz::le64(p + k - 8u) == k) {
                const uint64_t left = avail - k;
                if (left < kHeaderBytes && magic_prefix(p + k, left) && (left < 5u || p[k + 4u] == 1u)) return member(p, k, it);
                return it.at = base + k, it.error(kTrailing);
            }
        return it.error(kRanOut);
    }

    void take(const Item& it) {
        if (it.kind == MemberItem) ++members, searched = 0;
        else
            searched = it.searched;
    }

private:
    static Item& member(const uint8_t* p, uint64_t q, Item& it) {
        it.kind = MemberItem;
        it.bytes = q;
        it.trailer = member_trailer(p + q - kTrailerBytes);
        return it;
    }
};

}  // namespace lzip
}  // namespace slimm
