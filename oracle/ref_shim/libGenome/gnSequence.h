/* Stand-in for libGenome's sequence class, backed by a std::string.
   Coordinates follow libGenome: ToArray and ToString offsets are 1-based. */
#ifndef MUMS_REF_SHIM_GNSEQUENCE_H
#define MUMS_REF_SHIM_GNSEQUENCE_H
#include "libGenome/gnDefs.h"
#include "libGenome/gnClone.h"
#include "libGenome/gnException.h"
#include "libGenome/gnDebug.h"

namespace genome {

class gnGenomeSpec {
public:
	std::string GetName() const { return m_name; }
	std::string GetSourceName() const { return m_name; }
	void SetName(const std::string& n) { m_name = n; }
private:
	std::string m_name;
};

class gnSequence : public gnClone {
public:
	gnSequence() : m_circular(false) {}
	gnSequence(const gnSeqC* s) : m_seq(s), m_circular(false) {}
	gnSequence(const std::string& s) : m_seq(s), m_circular(false) {}
	virtual ~gnSequence() {}
	virtual gnSequence* Clone() const { return new gnSequence(*this); }

	virtual gnSeqI length() const { return m_seq.size(); }
	virtual gnSeqI size() const { return m_seq.size(); }
	virtual boolean isCircular() const { return m_circular; }
	virtual void setCircular(boolean c) { m_circular = c; }

	/* Copies up to len characters starting at 1-based offset; len is updated
	   to the count actually copied. */
	virtual boolean ToArray(gnSeqC* dest, gnSeqI& len, const gnSeqI offset = 1, const uint32 = ALL_CONTIGS) const {
		gnSeqI start = offset == 0 ? 0 : offset - 1;
		if (start > m_seq.size())
			start = m_seq.size();
		gnSeqI n = std::min<gnSeqI>(len, m_seq.size() - start);
		std::memcpy(dest, m_seq.data() + start, n);
		len = n;
		return true;
	}
	/* Passing a temporary length is common in libMems. */
	virtual boolean ToArray(gnSeqC* dest, const gnSeqI& len, const gnSeqI offset = 1, const uint32 c = ALL_CONTIGS) const {
		gnSeqI n = len;
		return ToArray(dest, n, offset, c);
	}
	virtual std::string ToString(const gnSeqI len = GNSEQI_END, const gnSeqI offset = 1) const {
		gnSeqI start = offset == 0 ? 0 : offset - 1;
		if (start > m_seq.size())
			start = m_seq.size();
		return m_seq.substr(start, len);
	}
	virtual boolean ToString(std::string& str, const gnSeqI len = GNSEQI_END, const gnSeqI offset = 1) const {
		str = ToString(len, offset);
		return true;
	}
	virtual gnSequence subseq(const gnSeqI offset, const gnSeqI len) const {
		return gnSequence(ToString(len, offset));
	}
	virtual int compare(const gnSequence& o) const { return m_seq.compare(o.m_seq); }
	virtual int compare(const std::string& o) const { return m_seq.compare(o); }
	gnSequence& operator=(const std::string& s) { m_seq = s; return *this; }
	gnSequence& operator+=(const std::string& s) { m_seq += s; return *this; }
	gnSequence& operator+=(const gnSequence& s) { m_seq += s.m_seq; return *this; }

	virtual gnGenomeSpec* GetSpec() const { return &m_spec; }
	virtual uint32 contigListSize() const { return 1; }
	virtual uint32 contigListLength() const { return 1; }
	virtual gnSequence contig(const uint32) const { return *this; }
	virtual std::string contigName(const uint32) const { return m_spec.GetName(); }
	virtual void LoadSource(const std::string&) { Throw_gnEx(FileNotOpened()); }

protected:
	std::string m_seq;
	boolean m_circular;
	mutable gnGenomeSpec m_spec;
};

}  // namespace genome

#endif
