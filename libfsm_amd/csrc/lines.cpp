/*
 * lines.cpp -- the host half of the text front (text.hip): the description transform that makes a delimiter byte invisible
 * to an automaton, and the line matcher that owns the automaton built from it.
 *
 * A line never contains its delimiter, and every line but possibly the last is followed by exactly one.  Replace the
 * delimiter's column of the transition function by the identity -- delta'(s, delim) = s for every state; DEAD, the implicit
 * target of a missing edge, loops on every byte already -- and walking [off[i], off[i + 1]) of the UNTOUCHED text, trailing
 * delimiter included, ends in the state that walking the line alone ends in under delta.  State ids, end states, end-ids and
 * eager-output SETS are the same (a self-loop re-enters a state whose ids were emitted when it was entered); the ordered
 * emission stream is not (it sees the extra step), which is why the text front offers no trace.
 */
#include <algorithm>
#include <cerrno>
#include <cstdlib>
#include <cstring>
#include <new>
#include <vector>

#include "../../include/fsm_hip.h"
#include "flat.h"

namespace {

template <class T>
bool dup_array(T **dst, const T *src, size_t count)
{
	*dst = static_cast<T *>(malloc((count ? count : 1) * sizeof(T)));   /* never NULL for an empty array: NULL means "none" */
	if (*dst == nullptr) return false;
	if (count != 0) memcpy(*dst, src, count * sizeof(T));
	return true;
}

}   // namespace

extern "C" struct fsm_hip_dfa_desc *fsm_hip_desc_identity_byte(const struct fsm_hip_dfa_desc *desc, int byte)
{
	if (desc == nullptr || byte < 0 || byte > 255 || desc->nstates == 0 || desc->start >= desc->nstates ||
	    desc->edge_off == nullptr || desc->is_end == nullptr || (desc->edge_off[desc->nstates] != 0 && desc->ranges == nullptr) ||
	    (desc->endid_off != nullptr && desc->endid_off[desc->nstates] != 0 && desc->endids == nullptr) ||
	    (desc->eager_off != nullptr && desc->eager_off[desc->nstates] != 0 && desc->eager_ids == nullptr)) {
		errno = EINVAL;
		return nullptr;
	}
	const uint32_t S = desc->nstates;
	const uint8_t b = (uint8_t)byte;
	std::vector<uint32_t> eoff;
	std::vector<fsm_hip_range> out, row;
	try {
		eoff.reserve((size_t)S + 1);
		out.reserve((size_t)desc->edge_off[S] + 2u * S);
		eoff.push_back(0);
		for (uint32_t s = 0; s < S; s++) {
			if (desc->edge_off[s] > desc->edge_off[s + 1]) { errno = EINVAL; return nullptr; }
			row.clear();
			for (uint32_t k = desc->edge_off[s]; k < desc->edge_off[s + 1]; k++) {
				const fsm_hip_range &r = desc->ranges[k];
				if (r.lo > r.hi || r.to >= S) { errno = EINVAL; return nullptr; }
				/* what the range keeps beside `byte`: the part below it and the part above it */
				if (r.lo < b) row.push_back(fsm_hip_range{r.lo, (uint8_t)std::min<unsigned>(r.hi, b - 1u), 0, r.to});
				if (r.hi > b) row.push_back(fsm_hip_range{(uint8_t)std::max<unsigned>(r.lo, b + 1u), r.hi, 0, r.to});
			}
			row.push_back(fsm_hip_range{b, b, 0, s});
			std::sort(row.begin(), row.end(), [](const fsm_hip_range &x, const fsm_hip_range &y) { return x.lo < y.lo; });
			const size_t first = out.size();
			for (const fsm_hip_range &r : row) {
				if (out.size() > first) {
					fsm_hip_range &p = out.back();
					if (r.lo <= p.hi) { errno = EINVAL; return nullptr; }   /* overlapping ranges: not a DFA */
					if (r.lo == p.hi + 1u && r.to == p.to) { p.hi = r.hi; continue; }
				}
				out.push_back(r);
			}
			eoff.push_back((uint32_t)out.size());
		}
	} catch (const std::bad_alloc &) {
		errno = ENOMEM;
		return nullptr;
	}

	struct flat *f = static_cast<struct flat *>(calloc(1, sizeof *f));
	if (f == nullptr) { errno = ENOMEM; return nullptr; }
	bool ok = dup_array(&f->edge_off, eoff.data(), eoff.size()) && dup_array(&f->ranges, out.data(), out.size()) &&
	          dup_array(&f->is_end, desc->is_end, S);
	if (ok && desc->endid_off != nullptr)
		ok = dup_array(&f->endid_off, desc->endid_off, (size_t)S + 1) && dup_array(&f->endids, desc->endids, desc->endid_off[S]);
	if (ok && desc->eager_off != nullptr)
		ok = dup_array(&f->eager_off, desc->eager_off, (size_t)S + 1) && dup_array(&f->eager_ids, desc->eager_ids, desc->eager_off[S]);
	if (!ok) {
		fsm_hip_desc_free(&f->d);
		errno = ENOMEM;
		return nullptr;
	}
	f->d.nstates = S;
	f->d.start = desc->start;
	f->d.edge_off = f->edge_off;
	f->d.ranges = f->ranges;
	f->d.is_end = f->is_end;
	f->d.endid_off = f->endid_off;
	f->d.endids = f->endids;
	f->d.eager_off = f->eager_off;
	f->d.eager_ids = f->eager_ids;
	return &f->d;
}

/* ---- the line matcher: the twin automaton and the delimiter it was built for ---- */

struct fsm_hip_lines_dfa {
	struct fsm_hip_dfa *inner;
	int delim;
};

extern "C" struct fsm_hip_lines_dfa *fsm_hip_lines_dfa_create(const struct fsm_hip_dfa_desc *desc, int delim, unsigned flags)
{
	struct fsm_hip_dfa_desc *twin = fsm_hip_desc_identity_byte(desc, delim);
	if (twin == nullptr) return nullptr;
	struct fsm_hip_lines_dfa *ld = static_cast<struct fsm_hip_lines_dfa *>(malloc(sizeof *ld));
	if (ld == nullptr) {
		fsm_hip_desc_free(twin);
		errno = ENOMEM;
		return nullptr;
	}
	ld->delim = delim;
	ld->inner = fsm_hip_dfa_create(twin, flags);
	const int e = errno;
	fsm_hip_desc_free(twin);
	if (ld->inner == nullptr) {
		free(ld);
		errno = e;
		return nullptr;
	}
	return ld;
}

extern "C" const struct fsm_hip_dfa *fsm_hip_lines_dfa_inner(const struct fsm_hip_lines_dfa *ld)
{
	return ld == nullptr ? nullptr : ld->inner;
}

extern "C" int fsm_hip_lines_dfa_delim(const struct fsm_hip_lines_dfa *ld)
{
	if (ld == nullptr) { errno = EINVAL; return -1; }
	return ld->delim;
}

extern "C" void fsm_hip_lines_dfa_free(struct fsm_hip_lines_dfa *ld)
{
	if (ld == nullptr) return;
	fsm_hip_dfa_free(ld->inner);
	free(ld);
}
