/* Stand-in for libGenome's exception type, its code objects and throw macros. */
#ifndef MUMS_REF_SHIM_GNEXCEPTION_H
#define MUMS_REF_SHIM_GNEXCEPTION_H
#include "libGenome/gnDefs.h"
#include <exception>
#include <string>

namespace genome {

class gnExceptionCode {
public:
	gnExceptionCode(uint32 code, const char* name) : m_code(code), m_name(name) {}
	bool operator==(const gnExceptionCode& o) const { return m_code == o.m_code; }
	bool operator!=(const gnExceptionCode& o) const { return m_code != o.m_code; }
	uint32 GetInt() const { return m_code; }
	const std::string& GetName() const { return m_name; }
private:
	uint32 m_code;
	std::string m_name;
};

inline uint32& gnNextExceptionCode() {
	static uint32 next = 0;
	return next;
}

class gnException : public std::exception {
public:
	gnException(const char* file, unsigned line, const char* func, const gnExceptionCode& code,
	            const std::string& msg = std::string())
		: m_code(code), m_msg(msg) {
		m_what = code.GetName() + " at " + file + ":" + std::to_string(line) + " in " + func;
		if (!msg.empty())
			m_what += ": " + msg;
	}
	virtual ~gnException() throw() {}
	const gnExceptionCode& GetCode() const { return m_code; }
	const std::string& GetMessage() const { return m_msg; }
	void AddCaller(const char*, unsigned, const char*) {}
	virtual const char* what() const throw() { return m_what.c_str(); }
private:
	gnExceptionCode m_code;
	std::string m_msg;
	std::string m_what;
};

inline std::ostream& operator<<(std::ostream& os, const gnException& e) {
	return os << e.what() << "\n";
}

}  // namespace genome

#define CREATE_EXCEPTION(E) \
	inline genome::gnExceptionCode& E() { \
		static genome::gnExceptionCode* code = new genome::gnExceptionCode(genome::gnNextExceptionCode()++, #E); \
		return *code; \
	}

namespace genome {
CREATE_EXCEPTION(NullPointer)
CREATE_EXCEPTION(IndexOutOfBounds)
CREATE_EXCEPTION(SeqIndexOutOfBounds)
CREATE_EXCEPTION(FragmentIndexOutOfBounds)
CREATE_EXCEPTION(FileNotOpened)
CREATE_EXCEPTION(FileUnreadable)
CREATE_EXCEPTION(IOStreamFailed)
CREATE_EXCEPTION(InvalidBaseQuality)
}

#define Throw_gnEx(code) throw genome::gnException(__FILE__, __LINE__, __func__, code)
#define Throw_gnExMsg(code, msg) throw genome::gnException(__FILE__, __LINE__, __func__, code, msg)
#define STACK_TRACE_START try {
#define STACK_TRACE_END } catch (genome::gnException& e) { e.AddCaller(__FILE__, __LINE__, __func__); throw; }

#endif
